"""Seeded inputs of the evaluation-matcher tests (tests/test_cpu_rbox.py, tests/test_oracle_rbox.py, tests/test_gpu_match.py) and
their oracle results, computed once per process and never modified.

`eval_match_coco` (csrc/eval_match.hip) picks one of four kernels by the number of ground truths G; the shapes are chosen around
their constants:

    G 1..64        match_coco_small_kernel<1>   taken set = one 64-bit mask          register blocks of RB detections
    G 65..256      match_coco_small_kernel<4>   four masks, ties -> highest chunk    register blocks of RB detections
    G 257..2048    match_coco_kernel<REG>       one bit per 64-gt chunk in a lane    ring of PF rows
    G 2049..2^20   match_coco_kernel<LDS>       bitmask in LDS (> 48 KiB: opt-in)    ring of PF rows

and every kernel writes its results as 64-detection stores plus a tail store."""
import collections
import functools

import numpy as np

import oracle

RB, PF, STORE, CHUNK = 32, 8, 64, 64
G_MAX = 1 << 20
LDS_OPT_IN_G = 393185      # first G whose taken bitmask (ceil(G / 32) + 1 words) exceeds 48 KiB of LDS
KINDS = ('dense', 'sparse', 'dist')

Case = collections.namedtuple('Case', 'path G D T kind special large')
Case.id = property(lambda c: f'{c.path}-G{c.G}-D{c.D}-T{c.T}-{c.kind}' + ('-infnan_thrs' if c.special else ''))
Case.seed = property(lambda c: c.G * 131 + c.D * 7 + KINDS.index(c.kind))


def path_of(G):
    return 'small1' if G <= 64 else 'small4' if G <= 256 else 'reg' if G <= 2048 else 'lds'


# (G, D, T, kind).  D against RB and the 64-wide store for the small kernels (1, 31 | 32 | 33, 64, 96 = a multiple of 32 but not of
# 64, 129), against PF and the store for the generic ones (1, 7 | 8 | 9, 63 | 64 | 65, 72 = a multiple of 8 past a store, 130).
# Every G comes with two D at least and two kinds at least; T = 4 marks the case whose thresholds include +inf, -inf and NaN.
_TABLE = (
    (1, 1, 1, 'dense'), (1, 33, 2, 'dist'),
    (2, 31, 3, 'sparse'), (2, 64, 2, 'dense'),
    (63, 32, 2, 'dist'), (63, 129, 3, 'sparse'),
    (64, 96, 4, 'dense'), (64, 33, 2, 'sparse'),

    (65, 1, 1, 'sparse'), (65, 129, 2, 'dense'),
    (127, 31, 2, 'dist'), (127, 64, 3, 'sparse'),
    (128, 32, 3, 'dense'), (128, 96, 2, 'dist'),
    (129, 33, 2, 'sparse'), (129, 64, 4, 'dense'),
    (192, 96, 2, 'dist'), (192, 31, 3, 'sparse'),
    (193, 129, 2, 'dense'), (193, 32, 2, 'dist'),
    (255, 64, 3, 'sparse'), (255, 33, 2, 'dense'),
    (256, 129, 3, 'sparse'), (256, 96, 3, 'dist'),

    (257, 1, 2, 'dense'), (257, 64, 3, 'sparse'),
    (320, 7, 2, 'dist'), (320, 130, 2, 'dense'),
    (511, 8, 3, 'sparse'), (511, 65, 2, 'dist'),
    (512, 9, 2, 'dense'), (512, 72, 4, 'sparse'),
    (513, 63, 2, 'dist'), (513, 130, 3, 'sparse'),
    (1024, 64, 2, 'dense'), (1024, 7, 3, 'dist'),
    (2047, 65, 3, 'sparse'), (2047, 9, 2, 'dense'),
    (2048, 130, 3, 'sparse'), (2048, 72, 2, 'dist'),

    (2049, 1, 2, 'sparse'), (2049, 64, 3, 'dense'), (2049, 130, 2, 'dist'),
    (2080, 7, 2, 'dist'), (2080, 65, 4, 'sparse'),
    (4096, 8, 3, 'dense'), (4096, 72, 2, 'sparse'), (4096, 63, 2, 'dist'),
    (4097, 9, 2, 'dist'), (4097, 130, 3, 'sparse'),
)
CASES = tuple(Case(path_of(G), G, D, T, kind, T == 4, False) for G, D, T, kind in _TABLE)
# the last size at 48 KiB of LDS, the first above it, the documented maximum
LARGE_CASES = tuple(Case('lds', G, D, 2, 'dense', False, True)
                    for G, D in ((LDS_OPT_IN_G - 1, 70), (LDS_OPT_IN_G, 70), (G_MAX, 3)))
PATHS = ('small1', 'small4', 'reg', 'lds')
SMALL_D = (1, 31, 32, 33, 64, 96, 129)
GENERIC_D = (1, 7, 8, 9, 63, 64, 65, 72, 130)
PATH_SHAPES = {'small1': ((1, 2, 63, 64), SMALL_D), 'small4': ((65, 127, 128, 129, 192, 193, 255, 256), SMALL_D),
               'reg': ((257, 320, 511, 512, 513, 1024, 2047, 2048), GENERIC_D), 'lds': ((2049, 2080, 4096, 4097), GENERIC_D)}


def make(D, G, T, kind, seed):
    """-> cost f32 (D, G), thrs f32 (T), ignore bool (G), crowd bool (G).

    dense : round(-U(0, 1), 2), thresholds -linspace(0, 0.9, T): many exact ties, the taken set decides who gets what.
    sparse: about 6 non-zero entries round(-U(0.05, 1), 1) per row, the rest -0.0, thresholds -linspace(0.1, 0.9, T): most
            detections match nothing (the evaluation regime).  Four of the six fall on a pool of max(2, D // 2) columns spread evenly
            over the gts, as detections crowd around the same objects: crowd gts are matched again and ignore gts pick up what is left.
    dist  : round(U(0, 6), 1), thresholds linspace(0.5, 3, T) (distance-like, positive).
    All: about 1 % NaN, three each of +inf, -inf and -0.0 (once there are 64 entries), ignore with p = 0.3, crowd with p = 0.1.
    G >= 2 adds the plant: gts 0 and G - 1 are neither ignore nor crowd; rows 0 and 1 hold the strictly lowest finite cost of the
    matrix at column G - 1, row 2 holds it at columns 0 and G - 1, and row 1 holds NaN at column 0.  At a threshold that admits
    that cost detection 0 takes G - 1 (the top bit of the last mask word or chunk), detections 1 and 2 must read its taken bit back
    and leave it alone, and detection 2 falls to gt 0.  The plant rows keep -inf only on ignore gts, which lose to gt G - 1."""
    rng = np.random.default_rng(seed)
    n = D * G
    if kind == 'dense':
        cost = np.round(-rng.random((D, G), dtype=np.float32), 2)
        thrs = -np.linspace(0.0, 0.9, T)
    elif kind == 'sparse':
        cost = np.full((D, G), -0.0, np.float32)
        pool = np.unique(np.linspace(0, G - 1, max(2, D // 2)).round().astype(np.int64))
        cols = np.where(rng.random((D, 6)) < 2 / 3, pool[rng.integers(0, len(pool), (D, 6))], rng.integers(0, G, (D, 6)))
        cost[np.arange(D)[:, None], cols] = np.round(-rng.uniform(0.05, 1, (D, 6)), 1).astype(np.float32)
        thrs = -np.linspace(0.1, 0.9, T)
    elif kind == 'dist':
        cost = np.round(rng.uniform(0, 6, (D, G)), 1).astype(np.float32)
        thrs = np.linspace(0.5, 3.0, T)
    else:
        raise ValueError(kind)
    thrs = thrs.astype(np.float32)
    ign = rng.random(G) < 0.3
    crowd = rng.random(G) < 0.1
    flat = cost.reshape(-1)
    flat[rng.integers(0, n, n // 100)] = np.nan
    if n >= 64:
        for value in (np.inf, -0.0, -np.inf):
            at = rng.integers(0, n, 3)
            if value == -np.inf and G >= 2:
                at = at[(at // G >= 3) | ign[at % G] & (at % G != 0) & (at % G != G - 1)]
            flat[at] = value
    if G >= 2:
        ign[[0, G - 1]] = False
        crowd[[0, G - 1]] = False
        low = np.float32(flat[np.isfinite(flat)].min() - 1)
        cost[:2, G - 1] = low
        if D >= 2:
            cost[1, 0] = np.nan
        if D >= 3:
            cost[2, 0] = cost[2, G - 1] = low
    return cost, thrs, ign, crowd


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def build(case):
    """the inputs of a table case, uncached (the large cases are made, used and dropped)"""
    cost, thrs, ign, crowd = make(case.D, case.G, case.T, case.kind, case.seed)
    if case.special:    # one ordinary value next to +inf (admits every non-NaN cost), -inf (only -inf costs), NaN (admits nothing)
        thrs = np.asarray([thrs[1], np.inf, -np.inf, np.nan], np.float32)
    return _freeze(cost, thrs, ign, crowd)


@functools.lru_cache(maxsize=None)
def inputs(case):
    assert not case.large
    return build(case)


@functools.lru_cache(maxsize=None)
def expected(case):
    """oracle.match_coco of a non-large case: (T, D) int32"""
    return _freeze(oracle.match_coco(*inputs(case)))[0]


def witnesses(case, matched, args=None):
    """What the ORACLE's answer `matched` exercises, so that the table cannot quietly stop covering what it claims."""
    cost, thrs, ign, crowd = args if args is not None else inputs(case)
    hit = matched >= 0
    ties = crowd_repeats = 0
    for t in range(case.T):
        d = np.nonzero(hit[t])[0]
        m = matched[t, d]
        crowd_repeats += int((np.bincount(m, minlength=case.G)[crowd] > 1).sum())
        same = (cost[d] == cost[d, m][:, None]) & (ign[None, :] == ign[m][:, None])
        ties += int((same.sum(1) > 1).sum())
    plant = None
    if case.G >= 2:     # detection 0 holds G - 1 at some threshold, and detection 1 does not at that threshold
        rows = matched[:, 0] == case.G - 1
        plant = bool(rows.any() and (case.D < 2 or (matched[rows, 1] != case.G - 1).all())
                     and (case.D < 3 or (matched[rows, 2] == 0).all()))
    return dict(unmatched=float(1.0 - hit.mean()), n=hit.size, ignore_matches=int(ign[matched[hit]].sum()), crowd_repeats=crowd_repeats,
                chunks=len(np.unique(matched[hit] // CHUNK)), all_chunks=(case.G + CHUNK - 1) // CHUNK,
                last=bool((matched == case.G - 1).any()), first=bool((matched == 0).any()), ties=ties, plant=plant)
