"""numpy oracle of the SimOTA BEV assigner (tests/test_cpu_simota.py, tests/test_gpu_simota.py): the sequence include/gd3d.h spells
out for gd3d_simota_assign, restated in np.float32 with one correctly rounded ELEMENTWISE operation per step — the fixed-sequence
logarithm (`fx_logf`) operation by operation, the membership tests on tests/pib_ref.py's `fx_sincos`, the classification cost in
ascending class order, the two selections with their tie rules (equal costs to the lower prior index, a conflicted prior's equal
row costs to the lower gt index).  The one thing NOT restated is the clipping of two rotated rectangles: the IoU matrix is the
package's own `bbox_overlaps_3d` on CPU tensors, an op with tests of its own (tests/test_cpu_pvrcnn_sample.py).  Comparisons of the
library against this file are EXACT.

`CASES` are named batches at the smallest shapes where the kernels can still go wrong (see each builder's comment).
"""
import numpy as np
import torch

from pib_ref import fx_sincos

F = np.float32
U = np.uint32


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def fx_logf(x):
    """csrc/fx_log.h on an fp32 array, one fp32 operation per line"""
    x = _f32(x).copy()
    shape = x.shape
    x = x.reshape(-1)
    with np.errstate(all='ignore'):
        ix = x.view(U).copy()
        out = np.empty_like(x)
        zero = (ix << U(1)) == 0
        neg = (ix >> U(31)) != 0
        big = ~neg & (ix >= U(0x7f800000))
        sub = ~neg & ~zero & (ix < U(0x00800000))
        xs = np.where(sub, x * F(33554432.0), x).astype(np.float32)
        k = np.where(sub, -25, 0).astype(np.int64)
        jx = xs.view(U).astype(np.int64) + (0x3f800000 - 0x3f3504f3)
        k = k + (jx >> 23) - 127
        jx = (jx & 0x007fffff) + 0x3f3504f3
        m = jx.astype(U).view(np.float32)
        f = m - F(1.0)
        s = f / (F(2.0) + f)
        z = s * s
        w = z * z
        t1 = w * (F(0.40000972152) + w * F(0.24279078841))
        t2 = z * (F(0.66666662693) + w * F(0.28498786688))
        r = t2 + t1
        hfsq = F(0.5) * f * f
        dk = k.astype(np.float32)
        out = s * (hfsq + r) + dk * F(9.0580006145e-06) - hfsq + f + dk * F(6.9313812256e-01)
        assert out.dtype == np.float32
        out = np.where(big, x, out)
        out = np.where(neg, F(np.nan), out)
        out = np.where(zero, F(-np.inf), out)
    return out.astype(np.float32).reshape(shape)


def cost_key(c):
    """an unsigned that orders as the cost does: -0 == +0, NaN above everything"""
    c = _f32(c)
    with np.errstate(all='ignore'):
        u = (c + F(0.0)).astype(np.float32).view(U)
    key = np.where((u >> U(31)) != 0, ~u, u | U(0x80000000)).astype(np.uint64)
    return np.where(np.isnan(c), np.uint64(0xffffffff), key)


def iou_matrix(boxes, gts):
    import mmdet3d_gaussian_amd as amd
    if len(boxes) == 0 or len(gts) == 0:
        return np.zeros((len(boxes), len(gts)), np.float32)
    iou = amd.bbox_overlaps_3d(torch.from_numpy(_f32(boxes)), torch.from_numpy(_f32(gts))).numpy()
    with np.errstate(all='ignore'):
        return np.where(iou > 0, iou, F(0.0)).astype(np.float32)


def membership(xy, gts, radius):
    """-> in_gt, in_ct (P, G) bool"""
    xy, g = _f32(xy), _f32(gts)
    with np.errstate(all='ignore'):
        hx, hy = g[:, 3] * F(0.5), g[:, 4] * F(0.5)
        s, c = fx_sincos(-g[:, 6])
        sx = xy[:, None, 0] - g[None, :, 0]
        sy = xy[:, None, 1] - g[None, :, 1]
        lx = sx * c[None] + sy * (-s)[None]
        ly = sx * s[None] + sy * c[None]
        in_gt = (lx > -hx[None]) & (lx < hx[None]) & (ly > -hy[None]) & (ly < hy[None])
        in_ct = (np.abs(sx) < F(radius)) & (np.abs(sy) < F(radius))
    return in_gt, in_ct


def cls_cost(scores, labels):
    """scores (V, C), labels (G,) -> (V, G) fp32"""
    s = _f32(scores)
    C = s.shape[1]
    with np.errstate(all='ignore'):
        s = np.where(s >= 0, np.where(s <= 1, s, F(1.0)), F(0.0)).astype(np.float32)
        s = np.sqrt(s)
        la = np.maximum(fx_logf(s), F(-100.0))
        lb = np.maximum(fx_logf(F(1.0) - s), F(-100.0))
        t = (np.arange(C)[None, :] == np.asarray(labels, np.int64)[:, None]).astype(np.float32)      # (G, C)
        total = np.zeros((s.shape[0], len(labels)), np.float32)
        for c in range(C):
            total = total + (-(t[None, :, c] * la[:, None, c] + (F(1.0) - t[None, :, c]) * lb[:, None, c]))
    assert total.dtype == np.float32
    return total


def assign_sample(scores, boxes, xy, gts, labels, radius, topk, iou_w, cls_w, match_init, stats=None):
    """One sample -> gt_inds (P,) int64, labels (P,) int64, max_overlaps (P,) fp32, positives [(prior, gt)] ascending.
    xy may have FEWER rows than scores (a shared grid shorter than the sample): the rows beyond are background."""
    P, G = len(scores), len(gts)
    gt_inds = np.zeros(P, np.int64)
    out_labels = np.full(P, -1, np.int64)
    max_overlaps = np.full(P, F(-1e8), np.float32)
    if P == 0 or G == 0:
        return gt_inds, out_labels, max_overlaps, []
    rows = min(P, len(xy))
    in_gt, in_ct = membership(_f32(xy)[:rows, :2], gts, radius)
    cand = np.nonzero((in_gt | in_ct).any(1))[0]
    V = len(cand)
    if stats is not None:
        stats.setdefault('cand', []).append(cand)
    if V == 0:
        return gt_inds, out_labels, max_overlaps, []
    both = (in_gt & in_ct)[cand]
    iou = iou_matrix(_f32(boxes)[cand], gts)
    with np.errstate(all='ignore'):
        ic = -fx_logf(iou + F(1e-8))
        cost = cls_cost(_f32(scores)[cand], labels) * F(cls_w) + ic * F(iou_w)
        cost = np.where(both, np.where(cost < F(match_init), cost, F(match_init)), cost).astype(np.float32)
    key = cost_key(cost)
    Kc = min(topk, V)
    taken = np.zeros((V, G), bool)
    for g in range(G):
        top = np.sort(iou[:, g])[::-1][:Kc]
        total = F(0.0)
        with np.errstate(all='ignore'):
            for v in top:
                total = F(total + v)
        k = 1 if not total >= 1 else (Kc if total >= Kc else int(total))
        k = min(k, Kc)
        if stats is not None:
            stats.setdefault('sums', []).append(float(total))
        order = np.lexsort((cand, key[:, g]))[:k]
        if stats is not None and V > k:
            full = np.sort(key[:, g])
            stats['tie_at_k'] = stats.get('tie_at_k', 0) + int(full[k - 1] == full[k])
        taken[order, g] = True
    pos = []
    for v in np.nonzero(taken.any(1))[0]:
        if taken[v].sum() > 1:
            g = int(np.argmin(key[v]))            # the lowest gt among equal keys
            if stats is not None:
                stats['conflicts'] = stats.get('conflicts', 0) + 1
                stats['third'] = stats.get('third', 0) + int(not taken[v, g])
        else:
            g = int(np.argmax(taken[v]))
        n = int(cand[v])
        gt_inds[n] = g + 1
        out_labels[n] = int(labels[g])
        max_overlaps[n] = iou[v, g]
        pos.append((n, g))
    return gt_inds, out_labels, max_overlaps, pos


def segments(cnt, rows):
    """the clamped segments of include/gd3d.h: [(start, n)] per sample"""
    out, s = [], 0
    for c in cnt:
        n = max(0, min(int(c), rows - s))
        out.append((s, n))
        s += n
    return out


def assign_batch(scores, boxes, priors, gts, labels, pcnt, gcnt, g_cap, shared=False, radius=0.5, topk=10, iou_w=3.0, cls_w=1.0,
                 match_init=2.0, stats=None):
    """The stacked contract -> dict of numpy arrays as `simota_assign` returns them."""
    P, B, L = len(scores), len(pcnt), g_cap * topk
    out = dict(gt_inds=np.zeros(P, np.int64), labels=np.full(P, -1, np.int64), max_overlaps=np.full(P, F(-1e8), np.float32),
               pos_cnt=np.zeros(B, np.int32), pos_inds=np.full((B, L), -1, np.int64), pos_gt_inds=np.full((B, L), -1, np.int64))
    for b, ((p0, pn), (g0, gn)) in enumerate(zip(segments(pcnt, P), segments(gcnt, len(gts)))):
        gn = min(gn, g_cap)
        xy = _f32(priors)[:pn] if shared else _f32(priors)[p0:p0 + pn]
        gi, lb, mo, pos = assign_sample(scores[p0:p0 + pn], boxes[p0:p0 + pn], xy, gts[g0:g0 + gn], labels[g0:g0 + gn], radius, topk,
                                        iou_w, cls_w, match_init, stats)
        out['gt_inds'][p0:p0 + pn], out['labels'][p0:p0 + pn], out['max_overlaps'][p0:p0 + pn] = gi, lb, mo
        out['pos_cnt'][b] = len(pos)
        for r, (n, g) in enumerate(pos):
            out['pos_inds'][b, r], out['pos_gt_inds'][b, r] = p0 + n, g0 + g
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------

def _gts(rng, G, span):
    g = np.zeros((G, 7), np.float32)
    g[:, 0:2] = rng.uniform(0, span, (G, 2))
    g[:, 2] = rng.uniform(-1.5, -0.5, G)
    g[:, 3] = rng.uniform(1.5, 4.5, G)
    g[:, 4] = rng.uniform(1.0, 2.5, G)
    g[:, 5] = rng.uniform(1.2, 2.0, G)
    g[:, 6] = rng.uniform(-3.2, 3.2, G)
    return g


def sample(rng, P, G, C=3, span=12.0, trained=True, grid=None):
    """priors scattered over (or a grid on) [0, span]^2; a `trained` prediction is the nearest gt's box, jittered"""
    gts = _gts(rng, G, span)
    labels = rng.integers(0, C, G).astype(np.int64)
    if grid is not None:
        priors = grid
        P = len(grid)
    else:
        priors = np.concatenate([rng.uniform(0, span, (P, 2)), np.full((P, 1), 0.5)], 1).astype(np.float32)
    boxes = np.zeros((P, 7), np.float32)
    boxes[:, 0:2] = priors[:, 0:2] + rng.normal(0, 0.3, (P, 2))
    boxes[:, 2] = rng.uniform(-1.5, -0.5, P)
    boxes[:, 3:6] = rng.uniform(1.0, 4.0, (P, 3))
    boxes[:, 6] = rng.uniform(-3.2, 3.2, P)
    scores = rng.uniform(0, 1, (P, C)).astype(np.float32)
    if trained and G and P:
        d = ((priors[:, None, 0:2] - gts[None, :, 0:2]) ** 2).sum(-1)
        near = d.argmin(1)
        boxes = (gts[near] + rng.normal(0, 0.15, (P, 7))).astype(np.float32)
        scores = (scores * 0.2).astype(np.float32)
        scores[np.arange(P), labels[near]] = rng.uniform(0.5, 1.0, P)
    return dict(scores=_f32(scores), boxes=_f32(boxes), priors=_f32(priors), gts=_f32(gts), labels=labels)


def _case(samples, shared=False, **params):
    return dict(samples=samples, shared=shared, params=params)


def _sizes(topk):
    # P off the workgroup size (1, 65, 257, 1025: one and several chunks), G past a wave and past a 256-gt LDS tile
    rng = np.random.default_rng(100 + topk)
    return _case([sample(rng, 1, 1, span=2.0), sample(rng, 65, 2, span=4.0), sample(rng, 257, 65), sample(rng, 1025, 257, span=24.0)],
                 topk=topk)


def _few_candidates():
    # V below K: three priors near the one gt, the others far away
    rng = np.random.default_rng(7)
    s = sample(rng, 40, 1, span=3.0)
    s['priors'][:3, 0:2] = s['gts'][0, 0:2] + np.array([[0.1, 0.0], [-0.2, 0.1], [0.0, -0.3]], np.float32)
    s['priors'][3:, 0:2] += 100.0
    return _case([s], topk=10)


def _empties():
    # a sample with no gts, one with no priors and one with no candidates, in the middle of a batch
    rng = np.random.default_rng(8)
    a, no_gt, no_pri, no_cand, z = (sample(rng, 90, 5), sample(rng, 70, 0), sample(rng, 0, 4), sample(rng, 33, 3), sample(rng, 130, 6))
    no_cand['priors'][:, 0:2] += 500.0
    return _case([a, no_gt, no_pri, no_cand, z], topk=10)


def _identical_gts():
    # two identical gts: every match conflicts, and the row tie goes to the lower gt
    rng = np.random.default_rng(9)
    s = sample(rng, 200, 1, span=5.0)
    s['gts'] = np.repeat(s['gts'], 2, 0)
    s['labels'] = np.repeat(s['labels'], 2, 0)
    return _case([s], topk=10)


def _crowd(seed):
    # 40 gts crowded on 3 m x 3 m: conflicts, some of whose row minimum is a THIRD gt, one that did not take the prior
    rng = np.random.default_rng(seed)
    return _case([sample(rng, 80, 40, span=3.0)], topk=3)


def _dense_queue():
    # 4000 priors on 3 m x 3 m under 6 gts: some three thousand candidates, nearly all of which overlap every gt — the clipping queue
    # is drained in the middle of the list and in more than one chunk, the selection buffers are cut several times
    rng = np.random.default_rng(15)
    return _case([sample(rng, 4000, 6, span=3.0)], topk=10)


def _all_clamped():
    # every prior inside the one big gt and its centre, every cost above match_init: ties decide everything
    rng = np.random.default_rng(11)
    s = sample(rng, 300, 2, span=4.0, trained=False)
    s['gts'][:, 0:2] = 2.0
    s['gts'][:, 3:5] = 20.0
    return _case([s], topk=10, radius=10.0, match_init=0.25)


def _dynamic_k_edge():
    # a dynamic-k sum at an integer and within an ulp below it: axis-aligned predictions of half the gt's length have IoU 1/2 exactly;
    # four of them sum to 2.0 (k = 2); with one of the four 2^-21 shorter the sum is the float next below 2 (k = 1), with one 2^-20
    # longer the float next above (k = 2)
    gts = np.array([[0, 0, 0, 4, 2, 2, 0], [0, 50, 0, 4, 2, 2, 0], [0, 100, 0, 4, 2, 2, 0]], np.float32)   # x = 0: every corner exact
    boxes = np.zeros((12, 7), np.float32)
    boxes[:] = [0, 0, 0, 2, 2, 2, 0]
    boxes[4:8, 1], boxes[8:, 1] = 50, 100
    boxes[7, 3] = F(2.0) - F(2.0 ** -21)
    boxes[11, 3] = F(2.0) + F(2.0 ** -20)
    priors = np.zeros((12, 3), np.float32)
    priors[:, 0] = np.tile(np.array([-0.2, -0.1, 0.1, 0.2], np.float32), 3)
    priors[:, 1] = boxes[:, 1]
    scores = np.full((12, 2), 0.5, np.float32)
    return _case([dict(scores=scores, boxes=boxes, priors=priors, gts=gts, labels=np.array([0, 1, 0], np.int64))], topk=10)


def _faces():
    # priors exactly on a box face (strict: outside), next inside it, exactly center_radius away (strict: outside) and next inside
    gts = np.array([[0, 0, 0, 4, 2, 2, 0], [20, 0, 0, 0.5, 0.5, 2, 0]], np.float32)
    r = F(0.5)
    xs = [2.0, np.nextafter(F(2.0), F(0)), -2.0, 0.0, 0.5, np.nextafter(r, F(0)), 20.5, np.nextafter(F(20.5), F(0)), 20.25, 19.5]
    ys = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.25, 0.0]
    rng = np.random.default_rng(12)
    s = sample(rng, len(xs), 2)
    s['gts'], s['priors'][:, 0], s['priors'][:, 1] = gts, _f32(xs), _f32(ys)
    return _case([s], topk=3, radius=0.5)


def _hostile():
    # NaN, +-inf and 1e30 in boxes and priors; scores of NaN, -1 and 2; labels outside [0, C)
    rng = np.random.default_rng(13)
    s = sample(rng, 400, 9, span=6.0)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for i in range(60):       # a yaw is NaN or +-inf, never a huge finite value: fx_sincosf's quadrant is unspecified beyond 2^31 quarter turns
        s['boxes'][rng.integers(0, 400), rng.integers(0, 7 if i % 5 < 3 else 6)] = bad[i % 5]
    for i in range(20):
        s['priors'][rng.integers(0, 400), rng.integers(0, 2)] = bad[i % 5]
    for i, v in enumerate([np.nan, -1.0, 2.0, np.inf, -np.inf, 0.0, 1.0] * 8):
        s['scores'][rng.integers(0, 400), i % 3] = v
    s['gts'][1, 3] = np.nan
    s['gts'][2, 0] = np.inf
    s['gts'][3, 4] = 1e30
    s['gts'][4, 6] = -np.inf
    s['gts'][5, 5] = -1.0
    s['labels'][6], s['labels'][7] = -1, 3
    return _case([s, sample(rng, 100, 4)], topk=10)


def _shared(topk):
    # one grid for every sample (the usual case): 33 x 31 = 1023 priors
    rng = np.random.default_rng(14)
    ys, xs = np.meshgrid(np.linspace(0, 12, 31, dtype=np.float32), np.linspace(0, 12, 33, dtype=np.float32), indexing='ij')
    grid = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, 0.375, np.float32)], 1)
    return _case([sample(rng, 0, G, grid=grid, trained=t) for G, t in ((7, True), (0, True), (30, False), (3, True))], shared=True, topk=topk)


CASES = {
    'sizes_topk10': _sizes(10),
    'sizes_topk1': _sizes(1),
    'sizes_topk32': _sizes(32),
    'few_candidates': _few_candidates(),
    'empties': _empties(),
    'identical_gts': _identical_gts(),
    'crowd': _crowd(10),
    'all_clamped': _all_clamped(),
    'dense_queue': _dense_queue(),
    'dynamic_k_edge': _dynamic_k_edge(),
    'faces': _faces(),
    'hostile': _hostile(),
    'shared_grid': _shared(10),
    'shared_grid_topk32': _shared(32),
}


def stacked(case):
    """-> (scores, boxes, priors, gts, labels, pcnt, gcnt) of a case; priors is the one grid of a shared case"""
    s = case['samples']
    C = s[0]['scores'].shape[1]
    cat = lambda k, w, dt: np.concatenate([np.asarray(x[k], dt).reshape((-1,) + w) for x in s], 0)   # noqa: E731
    priors = s[0]['priors'] if case['shared'] else cat('priors', (3,), np.float32)
    return (cat('scores', (C,), np.float32), cat('boxes', (7,), np.float32), priors, cat('gts', (7,), np.float32), cat('labels', (), np.int64),
            np.array([len(x['scores']) for x in s], np.int32), np.array([len(x['gts']) for x in s], np.int32))


_EXPECTED = {}


def expected(name, g_cap=None, stats=None):
    """The oracle's result of a case in its list form (g_cap = the largest gt count) or with the stacked form's g_cap; computed once."""
    case = CASES[name]
    sc, bx, pr, gt, lb, pcnt, gcnt = stacked(case)
    if g_cap is None:
        g_cap = int(gcnt.max())
    key = (name, g_cap)
    if key not in _EXPECTED or stats is not None:
        p = case['params']
        _EXPECTED[key] = assign_batch(sc, bx, pr, gt, lb, pcnt, gcnt, g_cap, shared=case['shared'], radius=p.get('radius', 0.5),
                                      topk=p['topk'], match_init=p.get('match_init', 2.0), stats=stats)
    return _EXPECTED[key]
