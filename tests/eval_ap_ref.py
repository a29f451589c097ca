"""The flexible mAP's accumulate and per-frame stages restated for the tests (not part of the product):

* `literal_accumulate`   — mean_ap_flexible.py:130-148 line by line, with mmdet's average_precision(mode='area') and its Python loop
                           over every detection (`average_precision_area`); ties are left to numpy, so use it with distinct scores;
* `vector_accumulate`    — the definition of include/gd3d.h in vectorised numpy (np.maximum.accumulate), for large cases;
* `exact_accumulate`     — the same on fractions.Fraction (the fp64 quotients p_j, then everything exact), for small ones;
* `literal_single`       — mean_ap_flexible.py:37-128 over the oracle's affinities and matcher, INCLUDING its one-tp-array-per-class
                           aliasing (:90, :115-116, :124-126: every breakdown's tuple holds the LAST breakdown's true positives);
* `build_cases`          — the case table of the accumulate kernels, computed from the library's tile size and scan chunk: random
                           cases of K <= 4, then cases built from lists of group sizes (`_layout_case`), whose sorted layout is
                           known and whose conditions (which boundary falls where) are asserted when the table is built;
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
    """-> (rows, first): rows = the records of groups [0, K) in sorted order (group, then rank), first (K + 1,) = where each group's
    rows start in it.  One stable sort and one searchsorted: linear in n + K (an unoccupied group has first[k] == first[k + 1])."""
    K = case['K']
    order = rank_order(case['score'])
    g = case['group'][order].astype(np.int64)
    live = (g >= 0) & (g < K)
    order, g = order[live], g[live]
    by_group = np.argsort(g, kind='stable')
    return order[by_group], np.searchsorted(g[by_group], np.arange(K + 1))


def vector_accumulate(case):
    """-> num_det (K, T) int64, recall (K, T) fp64, ap (K, T) fp64 (the e_j summed by math.fsum: exact, rounded once), n_tp (K, T).
    Unoccupied groups keep their zeros."""
    import math
    K, T = case['K'], case['T']
    num_det = np.zeros((K, T), np.int64)
    recall = np.zeros((K, T))
    ap = np.zeros((K, T))
    n_tp = np.zeros((K, T), np.int64)
    tp, msk = unpack(case['tp'], T), unpack(case['msk'], T)
    sorted_rows, first = _group_rows(case)
    for k in np.nonzero(first[1:] > first[:-1])[0]:
        rows = sorted_rows[first[k]:first[k + 1]]
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
    sorted_rows, first = _group_rows(case)
    for k in range(K):
        rows = sorted_rows[first[k]:first[k + 1]]
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
    return cases + _layout_cases(R, chunk, big)       # (their own generator: the cases above keep their draws)


# ---- cases built from a list of group sizes: the sorted layout is known, and asserted -------------------------------------------------------

STRAY_GROUPS = (-1, None, 2 ** 31 - 1, -2 ** 31)     # None: K itself


def _layout_case(name, rng, sizes, T, K=None, ids=None, strays=0, tp=None, msk=None, num_gt=None, p_msk=0.8, big=False):
    """A case whose SORTED layout is given: group ids[i] (default i; ascending) holds sizes[i] rows, whose scores fall strictly inside
    the group, so row j of the layout is row j after the sort; `tp` / `msk` (default: random words) are given in that layout.  `strays`
    rows of groups {-1, K, 2^31 - 1, -2^31} are appended — they sort last — and all rows are shuffled.  case['bounds'] =
    np.cumsum(sizes): where the groups end in the sorted rows."""
    sizes = np.asarray(sizes, np.int64)
    ids = np.arange(len(sizes)) if ids is None else np.asarray(ids, np.int64)
    K = len(sizes) if K is None else K
    assert len(ids) == len(sizes) and (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < K and (sizes >= 0).all()
    n = int(sizes.sum())
    group = np.repeat(ids, sizes)
    within = np.arange(n) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    score = (1.0 - (within + 0.5) / np.repeat(sizes, sizes)).astype(np.float32)
    tp = _words(rng, n, T) if tp is None else np.asarray(tp, np.uint32)
    msk = _words(rng, n, T, p_msk) if msk is None else np.asarray(msk, np.uint32)
    assert len(tp) == len(msk) == n
    if strays:
        group = np.concatenate([group, [K if STRAY_GROUPS[i % 4] is None else STRAY_GROUPS[i % 4] for i in range(strays)]])
        score = np.concatenate([score, rng.uniform(0, 1, strays).astype(np.float32)])
        tp, msk = np.concatenate([tp, _words(rng, strays, T)]), np.concatenate([msk, _words(rng, strays, T, 0.9)])
    if num_gt is None:
        num_gt = rng.integers(0, 6, K)
        num_gt[ids] = rng.integers(0, np.maximum(2, sizes))
    perm = rng.permutation(n + strays)
    c = _case(name, group[perm], score[perm], tp[perm], msk[perm], num_gt, T)
    assert c['K'] == K
    c['bounds'], c['sizes'], c['big'] = np.cumsum(sizes), sizes, big
    # the layout is what the sort gives: inside a group the scores fall strictly
    live = np.nonzero((c['group'] >= 0) & (c['group'] < K))[0]
    back = live[np.lexsort((-c['score'][live].astype(np.float64), c['group'][live]))]
    assert np.array_equal(c['group'][back], np.repeat(ids, sizes)) and np.array_equal(c['tp'][back], tp[:n]) and np.array_equal(c['msk'][back], msk[:n])
    assert n == 0 or (np.diff(c['score'][back].astype(np.float64))[np.diff(c['group'][back]) == 0] < 0).all()
    return c


def _bit0(rng, flags, T, p=0.5):
    """words whose bit 0 is `flags` and whose other bits are random"""
    return (_words(rng, len(flags), T, p) & ~np.uint32(1)) | np.asarray(flags, bool).astype(np.uint32)


def _fill(rng, rows, R):
    """group sizes of 3 to 4 tiles that add up to `rows` (the last two: what is left, halved)"""
    out = []
    while rows > 8 * R:
        out.append(int(rng.integers(3 * R, 4 * R + 1)))
        rows -= out[-1]
    assert rows >= 2
    return out + [rows // 2, rows - rows // 2]


def _has(bounds, lo, hi):
    """a group ends at a row of [lo, hi)"""
    return bool(((bounds >= lo) & (bounds < hi)).any())


def _layout_cases(R, chunk, big):
    rng = np.random.default_rng(20270)
    W = R // 4                 # rows of a wave: thread i of a tile holds rows 4i .. 4i + 3, wave w rows W w .. W w + W - 1
    assert R % 4 == 0 and W % 4 == 0
    cases = []
    # many boundaries per thread, per wave and per tile, at every alignment
    dense = [1, 2, 3, 4, 5, 6, 7, 1, 1, 2, 2, 3, 3] * 40
    seen_mod4 = set()
    for shift in range(5):
        c = _layout_case(f'segments_dense_shift{shift}', rng, [shift] + dense + [R + 3, 2, R, 1], 3, strays=37)
        b = c['bounds']
        lo, hi = shift, shift + sum(dense)
        seen_mod4 |= set((b[(b > lo) & (b <= hi)] % 4).tolist())
        sorted_groups = np.repeat(np.arange(c['K']), c['sizes'])
        quads = sorted_groups[:len(sorted_groups) // 4 * 4].reshape(-1, 4)
        assert ((np.diff(quads, axis=1) != 0).sum(1) >= 2).any(), 'no thread holds three groups'
        spans = [w for w in range(hi // W) if w * W >= lo and (w + 1) * W <= hi]
        assert len(spans) >= 4 and all(((b > w * W) & (b < (w + 1) * W)).sum() >= 8 for w in spans)
        cases.append(c)
    assert seen_mod4 == {0, 1, 2, 3}
    cases.append(_layout_case('singletons', rng, [1] * (2 * R + 5), 2, strays=11))
    c = _layout_case('wave_edge_boundaries', rng, [W, W, 2 * W, 3 * W, 1, W - 1, W // 4, 3 * W // 4, W - 1, 1, W + 1, W - 2, 1, 100], 3, strays=5)
    b = c['bounds']
    assert ((b % W == 0) & (b % R != 0)).sum() >= 4 and (b % W == 1).sum() >= 2 and (b % W == W - 1).sum() >= 2
    assert {int(x) // W % 4 for x in b[(b % W == 0) & (b % R != 0)]} == {1, 2, 3}       # each of a tile's three inner wave edges
    cases.append(c)
    c = _layout_case('tile_edge_paths', rng, [R // 2, R - R // 2, R, 5, R - 5, R // 3, 2 * R - R // 3, 7], 3, strays=9)
    s, e = c['bounds'] - c['sizes'], c['bounds']
    assert s[1] % R != 0 and e[1] % R == 0 and s[1] // R == (e[1] - 1) // R                     # mid-tile to exactly the tile's end
    assert s[2] % R == 0 and e[2] - s[2] == R and c['sizes'][1] > 0 and c['sizes'][3] > 0      # a whole tile between two others
    assert s[3] % R == 0 and e[3] % R != 0 and s[3] // R == e[3] // R                           # a tile's first row to mid-tile
    assert s[6] % R != 0 and e[6] % R == 0 and (e[6] - 1) // R == s[6] // R + 1                 # mid-tile to the end of the next tile
    cases.append(c)
    # groups longer than the 64 tiles one trip of the finish kernel's lanes covers
    cases.append(_layout_case('group_over_64_tiles', rng, [10, 65 * R + 17, 5], 3, strays=21))
    cases.append(_layout_case('group_over_128_tiles', rng, [3, 129 * R + 1], 3, strays=6))
    for c in cases[-2:]:
        assert ((c['bounds'] - 1) // R - (c['bounds'] - c['sizes']) // R).max() + 1 > (64 if '64' in c['name'] else 128)
    # the same long group, false positives first and true positives in its last 1.5 R rows (bit 0); bit 1 adds one early true
    # positive whose precision 1/100 lies below the last one, so its envelope value comes from 64 tiles further on
    n0, n1, n2 = 33, 65 * R + 17, R // 2 + 3
    late = np.arange(n1) >= n1 - R - R // 2
    assert 1 / 100 < late.sum() / n1
    tp = np.concatenate([_words(rng, n0, 3), late.astype(np.uint32) * np.uint32(5) | (late | (np.arange(n1) == 99)).astype(np.uint32) * np.uint32(2),
                         (np.arange(n2) < n2 // 2).astype(np.uint32) * np.uint32(7)])
    cases.append(_layout_case('envelope_over_64_tiles', rng, [n0, n1, n2], 3, strays=13, tp=tp, msk=np.full(n0 + n1 + n2, 7, np.uint32),
                              num_gt=[9, n1, n2]))
    # every row a true positive at every threshold: whole tiles of e = 1, the top limb sums 2^31 per tile
    n0, n1 = 3 * R + 9, R // 4 + 1
    cases.append(_layout_case('all_true_positives', rng, [n0, n1], 3, strays=7, tp=np.full(n0 + n1, 7, np.uint32), msk=np.full(n0 + n1, 7, np.uint32),
                              num_gt=[n0, 0]))
    n0 = 2 * R + 3
    cases.append(_layout_case('one_true_positive_at_the_last_rank', rng, [n0], 3, strays=4, tp=(np.arange(n0) == n0 - 1).astype(np.uint32) * np.uint32(7),
                              msk=np.full(n0, 7, np.uint32), num_gt=[7]))
    for K in (1023, 1024, 1025):
        cases.append(_layout_case(f'groups_{K}', rng, rng.integers(1, 6, K), 1, strays=50))
        assert (cases[-1]['sizes'] > 0).all()
    K = 1 << 20
    ids = np.unique(np.concatenate([[0, 1, K // 2 - 1, K // 2, K - 2, K - 1], rng.integers(0, K, 300)]))
    sizes = rng.integers(1, 31, len(ids))
    sizes[-1] += 4900 - sizes.sum()
    c = _layout_case('max_groups', rng, sizes, 1, K=K, ids=ids, strays=100, num_gt=rng.integers(1, 5, K))
    assert len(c['score']) == 5000 and (sizes > 0).all() and (c['num_gt'] > 0).all() and len(ids) > 200
    cases.append(c)
    if not big:
        return cases
    # ---- the carry scans' second and third trips over live rows (no stray rows: the last tile is live) ----
    E1, E2 = chunk * R, 2 * chunk * R
    m = (E2 - R // 2) // (R + R // 2)
    assert R // 2 + m * (R + R // 2) == E2
    c = _layout_case('three_scan_trips_short_groups', rng, [R // 2] + [R + R // 2] * m + [7], 2, big=True)
    n = len(c['score'])
    assert n == E2 + 7 and (n + R - 1) // R == 2 * chunk + 1 and all(_has(c['bounds'], k * R, (k + 1) * R + 1) for k in range(2 * chunk + 1))
    cases.append(c)
    # a group over each chunk edge: [E - 2R - 7, E + 2R + 5), true positives in its last R rows (bit 0: the counts flow forward over
    # the edge); bit 1 adds one early true positive of precision 1/10, below the last one (its envelope flows backward over the edge)
    span = 4 * R + 12
    sizes = _fill(rng, E1 - 2 * R - 7, R) + [span]
    a1 = len(sizes) - 1
    sizes += _fill(rng, E2 - 2 * R - 7 - sum(sizes), R) + [span]
    a2 = len(sizes) - 1
    sizes += [3 * R + 1]
    nn = sum(sizes)
    starts = np.cumsum(sizes) - np.asarray(sizes)
    assert starts[a1] == E1 - 2 * R - 7 and starts[a2] == E2 - 2 * R - 7 and 1 / 10 < R / span
    flags0, flags1 = rng.uniform(0, 1, nn) < 0.5, rng.uniform(0, 1, nn) < 0.5
    mk = _words(rng, nn, 2)
    for a in (a1, a2):
        rows = np.arange(starts[a], starts[a] + span)
        flags0[rows] = rows >= starts[a] + span - R
        flags1[rows] = flags0[rows] | (rows == starts[a] + 9)
        mk[rows] = 3
    c = _layout_case('chunk_edge_straddled', rng, sizes, 2, tp=flags0.astype(np.uint32) | flags1.astype(np.uint32) << np.uint32(1), msk=mk, big=True)
    assert not _has(c['bounds'], E1 - 2 * R - 6, E1 + 2 * R + 5) and not _has(c['bounds'], E2 - 2 * R - 6, E2 + 2 * R + 5)
    assert _has(c['bounds'], E1 + 2 * R + 5, E1 + 2 * R + 6) and _has(c['bounds'], E2 + 2 * R + 5, E2 + 2 * R + 6)
    cases.append(c)
    # groups that end exactly on the chunk edges: the one before ends in false positives over whole tiles, the one after opens with
    # precision 1 — counts leaking forward or the envelope leaking backward change a result
    n_before, n_after = 3 * R + 100, R + 9
    sizes = _fill(rng, E1 - n_before, R) + [n_before, n_after]
    b1 = len(sizes) - 2
    sizes += _fill(rng, E2 - n_before - sum(sizes), R) + [n_before, n_after]
    b2 = len(sizes) - 2
    sizes += [2 * R + 1]
    nn = sum(sizes)
    starts = np.cumsum(sizes) - np.asarray(sizes)
    assert starts[b1] + n_before == E1 and starts[b2] + n_before == E2
    flags0 = rng.uniform(0, 1, nn) < 0.5
    mk = _words(rng, nn, 2)
    for b_ in (b1, b2):
        rows = np.arange(starts[b_], starts[b_] + n_before)
        flags0[rows] = ((rows - starts[b_]) % 7 == 3) & (rows - starts[b_] < 40)
        after = np.arange(starts[b_ + 1], starts[b_ + 1] + n_after)
        flags0[after] = after - starts[b_ + 1] < n_after // 2
        mk[rows] |= 1
        mk[after] |= 1
    c = _layout_case('chunk_edge_is_boundary', rng, sizes, 2, tp=_bit0(rng, flags0, 2), msk=mk, big=True)
    assert _has(c['bounds'], E1, E1 + 1) and _has(c['bounds'], E2, E2 + 1) and len(c['score']) > E2 + R
    cases.append(c)
    c = _random_case(f'size_{chunk * R + 1}_second_scan_trip_live', rng, chunk * R + 1, 3, 2, stray=False, round_to=4)
    c['big'] = True
    assert ((c['group'] >= 0) & (c['group'] < 3)).all() and len(c['score']) == chunk * R + 1
    cases.append(c)
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
