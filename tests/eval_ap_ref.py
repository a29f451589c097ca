"""The flexible mAP's accumulate and per-frame stages restated for the tests (not part of the product):

* `literal_accumulate`   — mean_ap_flexible.py:130-148 line by line, with mmdet's average_precision(mode='area') and its Python loop
                           over every detection (`average_precision_area`); ties are left to numpy, so use it with distinct scores;
* `vector_accumulate`    — the definition of include/gd3d.h in vectorised numpy (np.maximum.accumulate), for large cases;
* `exact_accumulate`     — the same on fractions.Fraction (the fp64 quotients p_j, then everything exact), for small ones;
* `literal_single`       — mean_ap_flexible.py:37-128 over the oracle's affinities and matcher, INCLUDING its one-tp-array-per-class
                           aliasing (:90, :115-116, :124-126: every breakdown's tuple holds the LAST breakdown's true positives);
* `build_cases`          — the case table of the accumulate kernels, computed from the library's tile size and scan chunk;
* `random_dataset`       — detections and annotations in the reference's format.
"""
from fractions import Fraction

import numpy as np


# ---- rank order and bit helpers -----------------------------------------------------------------------------------------------------

def rank_order(score):
    """Row indices in the header's rank order: NaN first, then descending score with -0 == +0, ties in ascending row index."""
    score = np.asarray(score, np.float32)
    nan = np.isnan(score)
    s = np.where(nan, 0.0, score.astype(np.float64))
    return np.lexsort((np.arange(len(score)), -s, ~nan))


def unpack(bits, T):
    """(n,) words -> (T, n) bool"""
    return ((np.asarray(bits).astype(np.int64)[None, :] >> np.arange(T)[:, None]) & 1).astype(bool)


def pack(flags):
    """(T, n) bool -> (n,) uint32"""
    flags = np.asarray(flags, bool)
    w = (np.int64(1) << np.arange(flags.shape[0], dtype=np.int64))[:, None]
    return (flags.astype(np.int64) * w).sum(0).astype(np.uint32)


# ---- the literal form ---------------------------------------------------------------------------------------------------------------

def average_precision_area(recalls, precisions):
    """mmdet.core.evaluation.mean_ap.average_precision(mode='area') for one scale, restated with its loop."""
    recalls = recalls[np.newaxis, :]
    precisions = precisions[np.newaxis, :]
    num_scales = recalls.shape[0]
    ap = np.zeros(num_scales, dtype=np.float32)
    zeros = np.zeros((num_scales, 1), dtype=recalls.dtype)
    ones = np.ones((num_scales, 1), dtype=recalls.dtype)
    mrec = np.hstack((zeros, recalls, ones))
    mpre = np.hstack((zeros, precisions, zeros))
    for i in range(mpre.shape[1] - 1, 0, -1):
        mpre[:, i - 1] = np.maximum(mpre[:, i - 1], mpre[:, i])
    for i in range(num_scales):
        ind = np.where(mrec[i, 1:] != mrec[i, :-1])[0]
        ap[i] = np.sum((mrec[i, ind + 1] - mrec[i, ind]) * mpre[i, ind + 1])
    return ap[0]


def literal_accumulate(num_gt, score, tp, bkd_msk, num_thrs, fp64_ap=False):
    """mean_ap_flexible.py:131-148 -> [(num_det, recall, mAP)] per threshold.  fp64_ap: the area before mmdet's fp32 store."""
    out = []
    rank = score.argsort()[::-1]
    tp = tp[:, rank]
    bkd_msk = bkd_msk[:, rank]
    for t in range(num_thrs):
        tpcumsum = tp[t, bkd_msk[t]].cumsum()
        num_det = len(tpcumsum)
        recall = tpcumsum / max(num_gt, 1e-7)
        precision = tpcumsum / np.arange(1, num_det + 1)
        if fp64_ap:
            mrec = np.concatenate(([0.0], recall, [1.0]))
            mpre = np.concatenate(([0.0], precision, [0.0]))
            for i in range(len(mpre) - 1, 0, -1):
                mpre[i - 1] = max(mpre[i - 1], mpre[i])
            ind = np.where(mrec[1:] != mrec[:-1])[0]
            m_ap = np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1])
        else:
            m_ap = average_precision_area(recall, precision)
        max_recall = recall.max() if len(recall) > 0 else 0
        out.append((num_det, max_recall, m_ap))
    return out


# ---- the definition, vectorised and exact ---------------------------------------------------------------------------------------------

def _group_rows(case):
    order = rank_order(case['score'])
    g = case['group'][order]
    return [order[g == k] for k in range(case['K'])]


def vector_accumulate(case):
    """-> num_det (K, T) int64, recall (K, T) fp64, ap (K, T) fp64 (the e_j summed by math.fsum: exact, rounded once), n_tp (K, T)"""
    import math
    K, T = case['K'], case['T']
    num_det = np.zeros((K, T), np.int64)
    recall = np.zeros((K, T))
    ap = np.zeros((K, T))
    n_tp = np.zeros((K, T), np.int64)
    tp, msk = unpack(case['tp'], T), unpack(case['msk'], T)
    for k, rows in enumerate(_group_rows(case)):
        den = float(case['num_gt'][k]) if case['num_gt'][k] > 0 else 1e-7
        for t in range(T):
            r = rows[msk[t, rows]]
            h = tp[t, r]
            c = np.cumsum(h)
            D = len(r)
            num_det[k, t] = D
            if D == 0:
                continue
            p = c / np.arange(1, D + 1)
            e = np.maximum.accumulate(p[::-1])[::-1]
            recall[k, t] = c[-1] / den
            ap[k, t] = math.fsum(e[h]) / den
            n_tp[k, t] = int(h.sum())
    return num_det, recall, ap, n_tp


def exact_accumulate(case):
    """-> ap (K, T) as Fractions: the fp64 quotients p_j (the definition rounds them), envelope, sum and division exact"""
    K, T = case['K'], case['T']
    tp, msk = unpack(case['tp'], T), unpack(case['msk'], T)
    out = [[Fraction(0)] * T for _ in range(K)]
    for k, rows in enumerate(_group_rows(case)):
        den = Fraction(int(case['num_gt'][k])) if case['num_gt'][k] > 0 else Fraction(1e-7)
        for t in range(T):
            r = rows[msk[t, rows]]
            h = tp[t, r]
            c = np.cumsum(h)
            p = [float(ci) / float(j + 1) for j, ci in enumerate(c)]
            s, e = Fraction(0), 0.0
            for j in range(len(p) - 1, -1, -1):
                e = max(e, p[j])
                if h[j]:
                    s += Fraction(e)
            out[k][t] = s / den
    return out


# ---- the case table -------------------------------------------------------------------------------------------------------------------

def _case(name, group, score, tp, msk, num_gt, T):
    num_gt = np.asarray(num_gt, np.int64)
    return dict(name=name, group=np.asarray(group, np.int32), score=np.asarray(score, np.float32), tp=np.asarray(tp, np.uint32),
                msk=np.asarray(msk, np.uint32), num_gt=num_gt, K=len(num_gt), T=T)


def _words(rng, n, T, p=0.5):
    w = np.zeros(n, np.uint64)
    for t in range(T):
        w |= (rng.uniform(0, 1, n) < p).astype(np.uint64) << np.uint64(t)
    return w.astype(np.uint32)


def _random_case(name, rng, n, K, T, stray=True, round_to=2, p_msk=0.8):
    group = rng.integers(-1 if stray else 0, K + (1 if stray else 0), n)      # -1 and K interleaved: rows that count for nothing
    score = rng.uniform(0, 1, n)
    if round_to is not None:
        score = np.round(score, round_to)
    # tp is drawn independently of msk: tp bits on rows whose msk bit is clear occur everywhere
    return _case(name, group, score, _words(rng, n, T), _words(rng, n, T, p_msk), rng.integers(0, max(2, n // max(K, 1)), K), T)


def _sized_groups(sizes):
    return np.concatenate([np.full(s, g, np.int32) for g, s in enumerate(sizes)]) if sum(sizes) else np.zeros(0, np.int32)


def build_cases(R, chunk, big=True):
    """The accumulate kernels' cases for a tile of R sorted rows and carry scans of `chunk` tiles per trip."""
    rng = np.random.default_rng(20260)
    cases = []
    for n in (0, 1, R - 1, R, R + 1, 2 * R + 1, 3 * R + 5):
        cases.append(_random_case(f'size_{n}', rng, n, 3, 2))
    if big:
        cases.append(_random_case(f'size_{chunk * R + 1}_second_scan_trip', rng, chunk * R + 1, 3, 2, round_to=4))
    cases.append(_random_case('one_group', rng, 2 * R + 7, 1, 1, stray=False))
    # a boundary exactly on a tile edge (group 0 fills the first tile) and one in the middle of a tile
    n0, n1, n2 = R, R // 2 + 3, R + 11
    g = _sized_groups([n0, n1, n2])
    n = len(g)
    perm = rng.permutation(n)
    cases.append(_case('boundary_on_tile_edge_and_mid_tile', g[perm], np.round(rng.uniform(0, 1, n), 3), _words(rng, n, 2), _words(rng, n, 2, 0.9),
                       [n0 // 3, n1, 0], 2))
    # a group over 4+ whole tiles whose best precision sits in its last tile: false positives first, true positives at the end
    n0, n1 = 37, 4 * R + 100
    g = _sized_groups([n0, n1])
    score = np.concatenate([rng.uniform(0, 1, n0), np.linspace(1.0, 0.0, n1)])
    tp = np.concatenate([_words(rng, n0, 1), (np.arange(n1) >= n1 - R - R // 2).astype(np.uint32)])
    cases.append(_case('best_precision_in_last_tile', g, score, tp, np.ones(n0 + n1, np.uint32), [5, n1], 1))
    # the converse: group 0 ends in false positives over whole tiles, group 1 opens with precision 1 (a leak would raise group 0's envelope)
    n0, n1 = 2 * R + R // 2, R + 9
    g = _sized_groups([n0, n1])
    score = np.concatenate([np.linspace(1.0, 0.0, n0), np.linspace(1.0, 0.0, n1)])
    tp = np.concatenate([(np.arange(n0) % 7 == 3) & (np.arange(n0) < 40), np.arange(n1) < n1 // 2]).astype(np.uint32)
    cases.append(_case('next_group_opens_with_precision_1', g, score, tp, np.ones(n0 + n1, np.uint32), [n0, n1], 1))
    # an empty group between two others and an empty last group
    n = R + 77
    g = rng.choice([0, 2], n)
    cases.append(_case('empty_groups', g, np.round(rng.uniform(0, 1, n), 2), _words(rng, n, 2), _words(rng, n, 2, 0.9), [40, 7, 55, 3], 2))
    # group 1 fully masked at threshold 0, not at threshold 1
    c = _random_case('group_masked_at_one_threshold', rng, 2 * R + 3, 3, 2)
    c['msk'][c['group'] == 1] &= np.uint32(2)
    cases.append(c)
    for T in (1, 2, 31, 32):
        c = _random_case(f'thresholds_{T}', rng, R + 130, 2, T)
        cases.append(c)
    assert (cases[-1]['msk'] >> np.uint32(31)).any() and (cases[-1]['tp'] >> np.uint32(31)).any()
    # scores
    c = _random_case('scores_all_equal', rng, 2 * R + 9, 2, 2)
    c['score'][:] = 0.25
    cases.append(c)
    c = _random_case('ties_straddling_tile_edges', rng, 3 * R + 1, 1, 2, stray=False)
    c['score'] = (np.arange(len(c['score'])) // (R // 2 + 1)).astype(np.float32)[rng.permutation(len(c['score']))]
    cases.append(c)
    c = _random_case('special_scores', rng, 2 * R + 50, 2, 2)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -1.5, -1e-3, 1e-40, -1e-40, 1.4e-45, 3.0e38], np.float32)
    c['score'] = special[rng.integers(0, len(special), len(c['score']))]
    c['score'][::5] = rng.uniform(-2, 2, len(c['score'][::5])).astype(np.float32)
    cases.append(c)
    # num_gt = 0 with true positives (group 0) and without (group 1)
    c = _random_case('num_gt_zero', rng, R + 40, 2, 2, stray=False)
    c['num_gt'][:] = 0
    c['tp'][c['group'] == 1] = 0
    cases.append(c)
    # the same records shuffled and pre-sorted (ties break by row index, so the two may differ from each other: each is held to the twin)
    c = _random_case('records_shuffled', rng, 2 * R + 300, 3, 2)
    cases.append(c)
    order = np.lexsort((-c['score'].astype(np.float64), c['group']))
    cases.append(_case('records_presorted', c['group'][order], c['score'][order], c['tp'][order], c['msk'][order], c['num_gt'], 2))
    return cases


def distinct_scores(rng, n):
    """n different fp32 scores in (0, 1)"""
    return ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)


# ---- the per-frame stage, literally -----------------------------------------------------------------------------------------------------

def _bkd_flags(bkd, boxes, attrs):
    """breakdown.py: NoBreakdown (bkd None) or RangeBreakdown (bkd = dict name -> (lo, hi))"""
    num_boxes = len(boxes)
    if bkd is None:
        flags = np.ones((1, num_boxes), dtype=bool)
    else:
        distance = np.linalg.norm(boxes[:, :3], axis=-1)
        flags = np.zeros((len(bkd), num_boxes), dtype=bool)
        for i, (lo, hi) in enumerate(bkd.values()):
            flags[i][(distance >= lo) & (distance < hi)] = True
    if attrs is not None and 'ignore' in attrs:
        flags[:, attrs['ignore']] = False
    return flags


def literal_single(det, anno, classes, breakdowns, affinity, match_thrs, z_offset=0.5):
    """mean_ap_flexible.py:37-128 with oracle.eval_* / oracle.match_coco in place of the compiled helpers.  breakdowns: a list of
    RangeBreakdown range dicts (NoBreakdown is put first, as the constructor does); affinity: 'iou3d' | 'ioubev' | 'trans'.
    Returns the tuples and, per class, the affinity matrix (None in the empty branch)."""
    import oracle
    bkds = [None] + list(breakdowns)
    negate = affinity != 'trans'
    thrs = np.array(match_thrs, np.float32)
    tp_score_info, affinities = [], []
    for cls in range(len(det)):
        cls_name = classes[cls]
        cls_det_bboxes = det[cls][:, :-1]
        cls_det_scores = det[cls][:, -1]
        sort_ind = cls_det_scores.argsort()[::-1]
        cls_det_bboxes = cls_det_bboxes[sort_ind]
        cls_det_scores = cls_det_scores[sort_ind]
        cls_num_dets = cls_det_scores.shape[0]
        cls_gt_msk = anno['gt_labels'] == cls
        cls_gt_bboxes = anno['gt_bboxes'][cls_gt_msk]
        cls_gt_attrs = {k: v[cls_gt_msk] for k, v in anno['gt_attrs'].items()}
        cls_num_ignore_gts = np.count_nonzero(cls_gt_attrs['ignore']) if 'ignore' in cls_gt_attrs else 0
        cls_num_gts = len(cls_gt_bboxes) - cls_num_ignore_gts
        cls_det_bkd = np.concatenate([_bkd_flags(b, cls_det_bboxes, None) for b in bkds], axis=0)
        cls_gt_bkd = np.concatenate([_bkd_flags(b, cls_gt_bboxes, cls_gt_attrs) for b in bkds], axis=0)
        cls_bkd_names = sum((['All'] if b is None else list(b) for b in bkds), [])
        num_bkd = cls_gt_bkd.shape[0]
        cls_tp = np.zeros((len(thrs), cls_num_dets), dtype=bool)            # ONE array, shared by every tuple below
        cls_gt_count = [np.count_nonzero(cls_gt_bkd[i]) for i in range(num_bkd)]
        if (cls_num_gts + cls_num_ignore_gts) == 0 or cls_num_dets == 0:
            affinities.append(None)
            for i in range(num_bkd):
                tp_score_info.append((cls_name, cls_bkd_names[i], cls_gt_count[i], cls_det_scores, cls_tp,
                                      cls_det_bkd[i:i + 1].repeat(len(thrs), axis=0)))
            continue
        aff = {'iou3d': lambda: oracle.eval_iou_3d(cls_det_bboxes, cls_gt_bboxes, z_offset),
               'ioubev': lambda: oracle.eval_iou_bev(cls_det_bboxes, cls_gt_bboxes),
               'trans': lambda: oracle.eval_trans_bev(cls_det_bboxes, cls_gt_bboxes)}[affinity]()
        affinities.append(aff)
        crowd = np.zeros(aff.shape[1], dtype=bool)
        for i in range(num_bkd):
            cls_gt_bkd_msk = cls_gt_bkd[i]
            matched_gt_idx = oracle.match_coco(-aff if negate else aff, -thrs if negate else thrs, ~cls_gt_bkd_msk, crowd)
            cls_tp[...] = False
            cls_tp[matched_gt_idx > -1] = True
            _msk_fp = cls_det_bkd[i:i + 1] & (matched_gt_idx == -1)
            _msk_tp = cls_gt_bkd_msk[matched_gt_idx] & (matched_gt_idx > -1)
            tp_score_info.append((cls_name, cls_bkd_names[i], cls_gt_count[i], cls_det_scores, cls_tp, _msk_fp | _msk_tp))
    return tp_score_info, affinities


def literal_eval(det_results, annotations, classes, breakdowns, affinity, match_thrs):
    """statistics_eval with nproc = 0 (:150-188) -> [(key, value)], value['mAP'] an np.float32 as mmdet returns"""
    infos = [literal_single(d, a, classes, breakdowns, affinity, match_thrs)[0] for d, a in zip(det_results, annotations)]
    out = []
    for item in zip(*infos):
        cls, bkd, num_gt, score, tp, msk = tuple(zip(*item))
        num_gt = sum(num_gt)
        res = literal_accumulate(num_gt, np.concatenate(score), np.concatenate(tp, axis=1), np.concatenate(msk, axis=1), len(match_thrs))
        for thr, (num_det, recall, m_ap) in zip(match_thrs, res):
            out.append((dict(class_name=cls[0], breakdown=bkd[0], match_threshold=thr),
                        dict(num_det=num_det, num_gt=num_gt, recall=recall, mAP=m_ap)))
    return out


def _boxes(rng, n, lim):
    return np.concatenate([rng.uniform(-lim, lim, (n, 2)), rng.uniform(-1.5, 0.5, (n, 1)), rng.uniform(1.2, 4.5, (n, 3)),
                           rng.uniform(-3.1, 3.1, (n, 1))], axis=1).astype(np.float32)


def random_dataset(seed, frames, num_cls, dets_per_frame, gts_per_frame, lim=60.0):
    """-> det_results[frame][cls] (n, 8) fp32 with dataset-wide distinct scores per class, annotations (gt_bboxes, gt_labels,
    gt_attrs['ignore']).  Some frames have no gt or no detection of a class."""
    rng = np.random.default_rng(seed)
    per_cls = [[] for _ in range(num_cls)]
    annotations = []
    for f in range(frames):
        G = 0 if f % 11 == 5 else int(rng.integers(1, 2 * gts_per_frame))
        gt = _boxes(rng, G, lim)
        labels = rng.integers(0, num_cls, G)
        annotations.append(dict(gt_bboxes=gt, gt_labels=labels, gt_attrs=dict(ignore=rng.uniform(0, 1, G) < 0.15)))
        for c in range(num_cls):
            mine = gt[labels == c]
            hit = mine[rng.uniform(0, 1, len(mine)) < 0.8].copy()
            hit[:, :2] += rng.normal(0, 0.25, (len(hit), 2))
            hit[:, 3:6] *= rng.uniform(0.9, 1.1, (len(hit), 3))
            hit[:, 6] += rng.normal(0, 0.08, len(hit))
            dup = hit[rng.uniform(0, 1, len(hit)) < 0.3].copy()
            dup[:, :2] += rng.normal(0, 0.3, (len(dup), 2))
            nfp = 0 if (f + c) % 13 == 7 else int(rng.integers(0, max(1, 2 * dets_per_frame // num_cls)))
            boxes = np.concatenate([hit, dup, _boxes(rng, nfp, lim)], axis=0).astype(np.float32)
            if (f + c) % 13 == 7:
                boxes = boxes[:0]
            per_cls[c].append(boxes[rng.permutation(len(boxes))])
    det_results = [[None] * num_cls for _ in range(frames)]
    for c in range(num_cls):
        scores = distinct_scores(rng, sum(len(b) for b in per_cls[c]))
        at = 0
        for f in range(frames):
            b = per_cls[c][f]
            det_results[f][c] = np.concatenate([b, scores[at:at + len(b), None]], axis=1).astype(np.float32)
            at += len(b)
    return det_results, annotations


def affinity_margin(affinities, match_thrs):
    """the smallest distance of any affinity to any threshold"""
    best = np.inf
    for a in affinities:
        if a is not None and a.size:
            best = min(best, float(np.abs(a[..., None].astype(np.float64) - np.asarray(match_thrs, np.float64)).min()))
    return best
