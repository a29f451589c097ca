"""TEST INFRASTRUCTURE: PV-RCNN's data path as ONE chain of the restatements tests/ already holds, and the cases of
tests/test_cpu_pvrcnn_chain.py and tests/test_gpu_pvrcnn_chain.py.

Every per-op suite compares one op with its restatement on inputs made for that op.  Here stage k of `oracle` consumes the oracle's
OWN stage k - 1 and never a product output, so what is compared at every stage boundary is the hand-off: the row layout (dead tail
rows, levels grouped by ascending sample), the counts, the stride passed three times per level, the truncation of a strided level,
`dense()` as the BEV map, the wrap-around of a short sample.

  A  voxelize              hard_voxel_ref.hard_voxelize_ref
  B  four sparse layers    sparse_conv_ref.index_ref + sparse_conv_ref.sparse_oracle, ReLU after each
  C  keypoints             vsa_bev_ref.get_voxel_centers / count_loop, the loop of `get_sampled_points` on vsa_ref.fps
  D  per-level pooling     vsa_ref.query_and_group;  voxel_query_ref.index_ref / coords_ref / query_ref / group_ref
  E  BEV                   vsa_bev_ref.interpolate_from_bev_features, in fp32 and in fp64
  F  RoI side              rpn_proposal_ref.expected, pvrcnn_sample_ref.restate (assign_one / sample_one), pib_ref.grid_points,
                           vsa_ref.query_and_group, pib_ref.mask_targets

Exactness: the weights are in {-1, 0, 1}, no bias, and the first level's features are integers (num_points and the voxel's z, y, x),
so every sum of B is an integer; the oracle asserts sum |x||w| < 2^24 for every output element, so the fp32 sum is exact IN ANY
ORDER and every comparison but E's is an equality.  The voxelizer's `mean` rides along as a second feature block of level 1 that D
only gathers.  E is compared as tests/test_cpu_vsa_bev.py compares `bev_interpolate` (vsa_bev_ref.check_values, its bound unchanged).

`case(variant)` builds the committed inputs, runs the oracle once and ASSERTS on the oracle's own outputs the conditions that keep the
case from being trivial (`_conditions`) — at import, for both variants (`CASES`); `FACTS[variant]` holds what it counted.  Nothing
here reads a product output; the one product call is the IoU matrix inside pvrcnn_sample_ref.restate, as in that op's own suite."""
import functools

import numpy as np
import torch

import hard_voxel_ref as hv
import pib_ref
import pvrcnn_sample_ref as ps
import rpn_proposal_ref as rp
import sparse_conv_ref as sc
import voxel_query_ref as vq
import vsa_bev_ref as vb
import vsa_ref

f32 = np.float32

# ---- the geometry: a grid of 16 x 16 x 8 cells, every centre exact in fp32 -------------------------------------------------------------
B = 3
VOXEL_SIZE = (0.5, 0.5, 0.25)
RANGE = (0.0, -4.0, -2.0, 8.0, 4.0, 0.0)
SHAPE = (8, 16, 16)                         # (D, H, W) = the grid as (z, y, x)
P, MV, WIDTH = 3, 128, 4                    # max_num_points, max_voxels, point columns
K = 48                                      # num_keypoints
CHANNELS = (4, 5, 6, 6, 4)                  # Cin of layer 1 = [num_points, z, y, x], then the four layers' Cout
LAYERS = (True, False, True, False)         # subm?  k3 everywhere; the strided layers are s2 p1
LEVELS = ((1, 0), (2, 2), (4, 3))           # (stride, the layer whose output is the level): strides 1, 2, 4
RADIUS = (0.75, 0.7, 1.3)                   # per level; 0.75^2 = 0.5625 = 0.5^2 + 0.5^2 + 0.25^2: a centre exactly ON the sphere exists
NSAMPLE = 3
MAX_RANGE = ((2, 2, 2), (0, 1, 1), (0, 1, 1))   # the voxel query's window (rz, ry, rx) per level.  Levels 2 and 3 are sorted by cell, so the
#                                             window walk meets the members in the ball query's row order: there the two ops differ
#                                             through the window (no z neighbours) and through d2 <= r2 against d2 < r2
ALIGNS = ('half', 'halfmin')
SOURCES = ('raw', 'vox')                    # keypoints from the raw points / from the voxel centres (`voxel_center_as_source`)
COUNTS = (300, 20, 150)                     # sample 1 has fewer points than K
VARIANTS = ('full', 'truncated')
SEED = 7
TRUNCATED_BY = 3                            # cells the truncating variant drops from the last level

# ---- stage F -----------------------------------------------------------------------------------------------------------------------------
HEAD = dict(H=6, W=7, A=2, C=3)
RPN_CFG = rp.cfg_of(40, 12, 12, nms_thr=0.5, score_thr=0.3)
SAMPLER = ps._sampler(8)
ASSIGNER = ps.SHIPPED
GRID = 3
ROI_RADIUS, ROI_NSAMPLE = 0.8, 3
ROI_FEATURES = ('raw', 'half', 2)           # the pooled ball features of D that are the keypoint features of F: source, align, stride
EXTRA_WIDTH = 0.2
FACTS = {}


def level_name(stride):
    return f's{stride}'


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def _draw_sample(rng, n, clusters):
    """n rows [x, y, z, intensity]: 70 % around `clusters` centres inside the anchors' region, the rest uniform over the range widened
    by 5 % (some fall outside and are dropped); intensity a multiple of 1/8"""
    lo, hi = np.asarray(RANGE[:3]), np.asarray(RANGE[3:])
    centres = np.stack([rng.uniform(1.0, 5.0, clusters), rng.uniform(-2.0, 2.0, clusters), rng.uniform(-1.6, -0.4, clusters)], 1)
    near = centres[rng.integers(0, clusters, n)] + rng.normal(0, 1, (n, 3)) * np.array([0.45, 0.45, 0.2])
    span = hi - lo
    far = lo - 0.05 * span + rng.random((n, 3)) * span * 1.1
    xyz = np.where((rng.random(n) < 0.7)[:, None], near, far)
    return np.concatenate([xyz, rng.integers(0, 8, (n, 1)) / 8.0], 1).astype(f32)


def make_points(seed, counts):
    rng = np.random.default_rng(seed)
    samples = [_draw_sample(rng, n, c) if n > 20 else
               np.concatenate([rng.uniform([2.0, -1.0, -1.5], [3.5, 0.5, -0.5], (n, 3)), rng.integers(0, 8, (n, 1)) / 8.0], 1).astype(f32)
               for n, c in zip(counts, (5, 1, 4))]
    return np.ascontiguousarray(np.concatenate(samples, 0)), np.asarray(counts, np.int32)


def make_weights(seed):
    """(27, Cin, Cout) in {-1, 0, 1}, half of them zero, per layer"""
    rng = np.random.default_rng(seed + 1000)
    return [rng.choice(np.array([-1, 0, 0, 1], f32), (27, cin, cout)) for cin, cout in zip(CHANNELS[:-1], CHANNELS[1:])]


@functools.lru_cache(maxsize=None)
def roi_inputs():
    """the head maps (sample 1 entirely under the score threshold), the oracle's own proposals, and gt boxes cut from them: two
    proposals of every non-empty sample nudged (IoU ~ 0.9: positives) and one box elsewhere; the sampler's two key tensors"""
    c = rp.make_inputs(SEED + 40, B, HEAD['H'], HEAD['W'], HEAD['A'], HEAD['C'])
    c['cls'][1] = -f32(2.0) - np.abs(c['cls'][1])
    prop = rp.expected(c['cls'], c['bbox'], c['dirp'], c['anchors'], RPN_CFG, HEAD['C'])
    rng = np.random.default_rng(SEED + 41)
    starts = np.concatenate(([0], np.cumsum(prop['batch_cnt'])))
    gts, glab = [], []
    for b in range(B):
        n = int(prop['batch_cnt'][b])
        rows = [starts[b] + i for i in (0, n // 2)] if n else []
        boxes = [prop['boxes_3d'][r] + f32([0.05, -0.04, 0.02, 0.03, 0.05, 0.02, 0.01]) for r in rows]
        labels = [int(prop['labels_3d'][r]) for r in rows]
        boxes.append(f32([rng.uniform(5.5, 7.0), rng.uniform(-3.5, 3.5), -1.6, 1.6, 3.9, 1.5, rng.uniform(-1, 1)]))
        labels.append(int(rng.integers(0, HEAD['C'])))
        gts.append(np.asarray(boxes, f32))
        glab.append(np.asarray(labels, np.int64))
    M = min(RPN_CFG['nms_post'], RPN_CFG['max_num'])
    keys = rng.random(B * M).astype(f32)
    fill = rng.random(B * SAMPLER['num']).astype(f32)
    c.update(gts=gts, glab=glab, keys=keys, fill_keys=fill, proposals=prop)
    return c


def make_inputs(seed, counts, max_out):
    """the points part of a case: points (N, 4), cnt (B,), the four layers' weights and the two strided layers' `max_out`"""
    points, cnt = make_points(seed, counts)
    return dict(points=points, cnt=cnt, weights=make_weights(SEED), max_out=tuple(int(m) for m in max_out))


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------

def _starts(cnt):
    return np.concatenate(([0], np.cumsum(np.asarray(cnt, np.int64))))


def first_features(num_points, coors):
    """what enters the first level: [num_points, z, y, x] as fp32, zero on dead rows"""
    x = np.concatenate([num_points[:, None], coors[:, 1:]], 1).astype(f32)
    return np.where((num_points > 0)[:, None], x, f32(0))


def sparse_layer(coors, shape, X, W, subm, max_out):
    """one layer + ReLU over the restated tables -> (index record, features (R, Cout) fp32); every sum exact in fp32 in any order"""
    index = sc.index_ref(coors, shape, B, 3, 1 if subm else 2, 1, subm, None if subm else max_out)
    zeros = np.zeros((len(index['nbr']), W.shape[2]))
    out = sc.sparse_oracle(index, X, W, None, zeros)['out']
    mag = sc.sparse_oracle(index, np.abs(X), np.abs(W), None, zeros)['out']
    assert mag.size == 0 or mag.max() < 2 ** 24, ('a sum of this layer is not exact in fp32', mag.max())
    assert np.array_equal(out, np.rint(out))
    return index, np.maximum(out, 0).astype(f32)


def centres(coors, stride, align):
    """-> (xyz (N, 3) fp32, cnt (B,) int32): get_voxel_centers and forward's count loop"""
    c = torch.from_numpy(np.ascontiguousarray(coors))
    xyz = vb.get_voxel_centers(c, VOXEL_SIZE, RANGE, stride, align)
    return xyz.numpy(), vb.count_loop(c, xyz, B).numpy()


def keypoints(xyz, cnt, num):
    """the loop of `get_sampled_points` on vsa_ref.fps, n < num wrapping as there; a sample WITHOUT points (the reference fails) takes
    the rows the op documents: local picks 0, the row offset clamped into the array"""
    st = _starts(cnt)
    out = np.zeros((len(cnt), num, 3), f32)
    for b, n in enumerate(int(v) for v in cnt):
        if n == 0:
            out[b] = xyz[min(st[b], len(xyz) - 1)]
            continue
        src = xyz[st[b]:st[b] + n]
        idx = vsa_ref.fps(src, num)
        if n < num:
            idx = np.tile(idx[:n], num // n + 1)[:num]
        out[b] = src[idx]
    return out


def table_of(skey, srow, shape):
    """the (B, Z, Y, X) table voxel_query_ref.query_ref walks, from the sorted index: of several rows in a cell the first (the lowest)"""
    cells = B * shape[0] * shape[1] * shape[2]
    table = np.full(cells, -1, np.int32)
    for k, r in zip(skey[::-1], srow[::-1]):
        if k < cells:
            table[k] = r
    return table.reshape((B,) + tuple(shape))


def ball_members(xyz, xyz_cnt, q, q_cnt, radius):
    """(M,) the uncapped member count of every ball (d2 < r2, the ball query's arithmetic)"""
    ps_, qb = _starts(xyz_cnt), vsa_ref.sample_of_rows(q_cnt)
    r2 = f32(radius) * f32(radius)
    return np.array([int((vsa_ref.dist2(q[m], xyz[ps_[b]:ps_[b] + int(xyz_cnt[b])]) < r2).sum()) for m, b in enumerate(qb)], np.int64)


def covered_query_and_group(radius, nsample, xyz, xyz_cnt, q, q_cnt, feats):
    """vsa_ref.query_and_group on the queries the counts cover; the rows past them are empty balls (zeros, idx 0), as the op documents"""
    m = int(np.sum(q_cnt))
    out, idx, _, mask = vsa_ref.query_and_group(radius, nsample, xyz, xyz_cnt, q[:m], q_cnt, feats)
    pad = len(q) - m
    return (np.concatenate([out, np.zeros((pad,) + out.shape[1:], f32)]), np.concatenate([idx, np.zeros((pad, nsample), np.int32)]),
            np.concatenate([mask, np.ones(pad, bool)]))


def oracle_points(inp, coords_scale=None):
    """stages A-E on the inputs of `make_inputs` -> (dict of numpy arrays under the keys of the product chain, facts).  `coords_scale`
    {stride: scale}: the scale handed to coords_ref for that level (the negative control of the tests)"""
    out, facts = {}, dict(empty_balls={}, crowded_balls={}, agree={}, differ={})
    cnt = inp['cnt']
    st = _starts(cnt)
    samples = [inp['points'][st[b]:st[b + 1]] for b in range(B)]
    # A
    a = hv.hard_voxelize_ref(samples, VOXEL_SIZE, RANGE, P, MV, WIDTH, WIDTH)
    for k in ('voxels', 'coors', 'num_points', 'voxel_batch_cnt', 'mean'):
        out[f'A.{k}'] = a[k]
    facts.update(voxels=int(a['num'][0]), dead_tail=len(a['coors']) - int(a['num'][0]), cut_samples=[], voxel_cnt=a['voxel_batch_cnt'].tolist())
    for b in range(B):
        cells, kept = hv.cells_of(samples[b], VOXEL_SIZE, RANGE)
        if len({tuple(c) for c in cells[kept]}) > MV:
            facts['cut_samples'].append(b)
    # B
    feats, coors, shape = first_features(a['num_points'], a['coors']), a['coors'], SHAPE
    out['B.in'] = feats
    layers = []
    for i, (subm, W) in enumerate(zip(LAYERS, inp['weights'])):
        index, feats = sparse_layer(coors, shape, feats, W, subm, None if subm else inp['max_out'][i // 2])
        coors, shape = index['out_coors'], tuple(index['out_shape'])
        layers.append(dict(indices=coors, features=feats, shape=shape, num=index['num'], cnt=index['out_batch_cnt'], kept=int(index['out_batch_cnt'].sum())))
        out[f'B.l{i}.indices'], out[f'B.l{i}.features'], out[f'B.l{i}.cnt'] = coors, feats, index['out_batch_cnt']
        if not subm:
            out[f'B.l{i}.num'] = index['num']
        assert shape == tuple(sc.out_shape_of(SHAPE, (1,) * 3, (LEVELS[(i + 1) // 2][0],) * 3, (0,) * 3)), (i, shape)
    facts.update(level_rows=[(layers[i]['kept'], len(layers[i]['indices'])) for _, i in LEVELS],
                 level_cnt=[layers[i]['cnt'].tolist() for _, i in LEVELS], last_total=int(layers[3]['num'][1]),
                 live_nonzero=[float((layers[i]['features'] != 0).any(1).sum()) / max(1, layers[i]['kept']) for _, i in LEVELS])
    # C
    xyz1, cnt1 = centres(a['coors'], 1, 'half')
    kps = dict(raw=keypoints(inp['points'][:, :3], cnt, K), vox=keypoints(xyz1, cnt1, K))
    out['C.raw.kp'], out['C.vox.kp'], out['C.vox.xyz'], out['C.vox.cnt'] = kps['raw'], kps['vox'], xyz1, cnt1
    key_cnt = np.full(B, K, np.int32)
    facts['wrap_picks'] = dict(raw=[max(0, K - int(n)) for n in cnt], vox=[max(0, K - int(n)) for n in cnt1])
    # D
    last = layers[LEVELS[-1][1]]
    dense = np.zeros((B, last['features'].shape[1]) + last['shape'], f32)
    live = (last['indices'] >= 0).all(1)
    lc = last['indices'][live]
    dense[lc[:, 0], :, lc[:, 1], lc[:, 2], lc[:, 3]] = last['features'][live]
    bev = dense.reshape(B, -1, last['shape'][1], last['shape'][2])
    out['E.bev'] = bev
    for align in ALIGNS:
        for stride, li in LEVELS:
            lv, radius, name, window = layers[li], RADIUS[LEVELS.index((stride, li))], level_name(stride), MAX_RANGE[LEVELS.index((stride, li))]
            xyz, xcnt = centres(lv['indices'], stride, align)
            assert np.array_equal(xcnt, lv['cnt'])
            f = np.concatenate([lv['features'], a['mean']], 1) if stride == 1 else lv['features']
            skey, srow = vq.index_ref(lv['indices'], lv['shape'], B)
            table = table_of(skey, srow, lv['shape'])
            out[f'D.{align}.{name}.xyz'], out[f'D.{align}.{name}.cnt'] = xyz, xcnt
            out[f'D.{name}.skey'], out[f'D.{name}.srow'] = skey, srow
            for src in SOURCES:
                q = kps[src].reshape(-1, 3)
                tag = f'D.{src}.{align}.{name}'
                g, idx, _, mask = vsa_ref.query_and_group(radius, NSAMPLE, xyz, xcnt, q, key_cnt, f)
                out[f'{tag}.ball.out'], out[f'{tag}.ball.idx'], out[f'{tag}.ball.pooled'] = g, idx, g.max(-1)
                scale = stride if coords_scale is None else coords_scale.get(stride, stride)
                nc = vq.coords_ref(q, key_cnt, VOXEL_SIZE, RANGE, scale)
                r = vq.query_ref(xyz, q, nc, table, window, radius, NSAMPLE)
                vg = vq.group_ref(xyz, q, f, r['idx'], r['cnt'], True)
                out[f'{tag}.voxel.coords'], out[f'{tag}.voxel.out'], out[f'{tag}.voxel.idx'], out[f'{tag}.voxel.pooled'] = nc, vg, r['idx'], vg.max(-1)
                members = ball_members(xyz, xcnt, q, key_cnt, radius)
                assert np.array_equal(members == 0, mask)
                same = (g.max(-1) == vg.max(-1)).all(1)
                for what, v in (('empty_balls', int(mask.sum())), ('crowded_balls', int((members > NSAMPLE).sum())),
                                ('agree', int((same & ~mask).sum())), ('differ', int((~same).sum()))):
                    facts[what][(align, stride)] = facts[what].get((align, stride), 0) + v
    # E
    for src in SOURCES:
        for align in ALIGNS:
            kp = torch.from_numpy(kps[src])
            b32 = torch.from_numpy(bev)
            out[f'E.{src}.{align}.interp'] = (vb.interpolate_from_bev_features(kp, b32, VOXEL_SIZE, RANGE, LEVELS[-1][0], align),
                                              vb.interpolate_from_bev_features(kp.double(), b32.double(), VOXEL_SIZE, RANGE, LEVELS[-1][0], align))
    return out, facts


def oracle_rois(kp, pooled):
    """stage F on the oracle's keypoints (B, K, 3) and their pooled features (B * K, C) -> (dict, facts)"""
    c = roi_inputs()
    out, facts = {}, {}
    prop = c['proposals']
    for k in ('boxes_3d', 'scores_3d', 'labels_3d', 'cls_preds', 'rois', 'batch_cnt'):
        out[f'F.prop.{k}'] = prop[k]
    pst = _starts(prop['batch_cnt'])
    t = torch.from_numpy
    case = dict(proposals=[t(prop['boxes_3d'][pst[b]:pst[b + 1]]) for b in range(B)],
                proposal_labels=[t(prop['labels_3d'][pst[b]:pst[b + 1]]) for b in range(B)],
                gt_bboxes=[t(g) for g in c['gts']], gt_labels=[t(g) for g in c['glab']], keys=t(c['keys']), fill_keys=t(c['fill_keys']),
                sampler=SAMPLER, assigner=ASSIGNER)
    s, _ = ps.restate(case)
    for k, v in s.items():
        out[f'F.sample.{k}'] = v.numpy()
    rois = s['rois'].numpy()
    grid = pib_ref.grid_points(rois[:, 1:], GRID).reshape(-1, 3)
    grid_cnt = np.array([(rois[:, 0] == b).sum() * GRID ** 3 for b in range(B)], np.int32)
    out['F.grid'], out['F.grid_cnt'] = grid, grid_cnt
    key_cnt = np.full(B, K, np.int32)
    flat = kp.reshape(-1, 3)
    g, idx, mask = covered_query_and_group(ROI_RADIUS, ROI_NSAMPLE, flat, key_cnt, grid, grid_cnt, pooled)
    out['F.ball.out'], out['F.ball.idx'] = g, idx
    T = max(len(g_) for g_ in c['gts'])
    boxes, labels = np.zeros((B, T, 7), f32), np.zeros((B, T), np.int64)
    for b in range(B):
        boxes[b, :len(c['gts'][b])], labels[b, :len(c['glab'][b])] = c['gts'][b], c['glab'][b]
    seg, box_idx = pib_ref.mask_targets(flat, key_cnt, boxes, labels, [len(g_) for g_ in c['gts']], EXTRA_WIDTH, HEAD['C'])
    out['F.seg'], out['F.box_idx'] = seg, box_idx
    covered = int(grid_cnt.sum())
    facts.update(pad_proposals=len(prop['rois']) - int(prop['batch_cnt'].sum()), proposal_cnt=prop['batch_cnt'].tolist(),
                 pos_cnt=s['pos_batch_cnt'].tolist(), roi_cnt=s['roi_batch_cnt'].tolist(), pad_rois=len(rois) - int(s['roi_batch_cnt'].sum()),
                 empty_grid_balls=int(mask[:covered].sum()), full_grid_balls=int((~mask[:covered]).sum()),
                 seg_classes=int(((seg >= 0) & (seg < HEAD['C'])).sum()), seg_background=int((seg == HEAD['C']).sum()), seg_ignored=int((seg == -1).sum()))
    return out, facts


def oracle(inp, with_roi=True, coords_scale=None):
    out, facts = oracle_points(inp, coords_scale)
    if with_roi:
        src, align, stride = ROI_FEATURES
        f_out, f_facts = oracle_rois(out[f'C.{src}.kp'], out[f'D.{src}.{align}.{level_name(stride)}.ball.pooled'])
        out.update(f_out)
        facts.update(f_facts)
    return out, facts


# ---- the committed cases -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _totals():
    """the true row counts of the two strided layers on the committed points: what the static `max_out`s are set around"""
    _, facts = oracle_points(make_inputs(SEED, COUNTS, (B * 4 * 8 * 8, B * 2 * 4 * 4)))
    return facts['level_rows'][1][0], facts['last_total']


def max_out_of(variant):
    """layer 2 keeps every row with room to spare (dead tail rows); the last layer holds every cell the grid has ('full') or
    TRUNCATED_BY fewer than the points reach ('truncated')"""
    total2, total4 = _totals()
    return total2 + 40, (B * 2 * 4 * 4 if variant == 'full' else total4 - TRUNCATED_BY)


def _conditions(variant, out, facts):
    """what keeps the case from being trivial, asserted on the oracle's own outputs"""
    for align in ALIGNS:
        for stride, _ in LEVELS:
            k = (align, stride)
            assert facts['empty_balls'][k] >= 1 and facts['crowded_balls'][k] >= 1, ('empty / crowded balls', k, facts['empty_balls'][k], facts['crowded_balls'][k])
            assert facts['agree'][k] >= 1 and facts['differ'][k] >= 1, ('ball query and voxel query', k, facts['agree'][k], facts['differ'][k])
    assert COUNTS[1] < K and facts['wrap_picks']['raw'][1] == K - COUNTS[1] and facts['wrap_picks']['vox'][1] > 0
    assert np.array_equal(out['C.raw.kp'][1, COUNTS[1]:], out['C.raw.kp'][1, :K - COUNTS[1]])
    assert facts['dead_tail'] >= 1 and len(facts['cut_samples']) >= 1, facts
    assert all(kept < rows for kept, rows in facts['level_rows'][:2]), 'levels 1 and 2 end in dead rows'
    assert min(facts['live_nonzero']) > 0.5, facts['live_nonzero']
    full = FACTS.get('full')
    if variant == 'truncated':
        assert full is not None
        lost = [a - b for a, b in zip(full['level_cnt'][2], facts['level_cnt'][2])]
        assert lost[0] == 0 and lost[2] >= 1 and sum(lost) == TRUNCATED_BY and facts['level_rows'][2][0] == facts['last_total'] - TRUNCATED_BY, lost
        facts['truncated_cells'] = lost
    else:
        assert facts['level_rows'][2][0] == facts['last_total'] < facts['level_rows'][2][1]
    assert facts['pad_proposals'] >= 1 and facts['pad_rois'] >= 1
    for b in range(B):
        if facts['proposal_cnt'][b]:
            assert facts['pos_cnt'][b] >= 1 and facts['roi_cnt'][b] - facts['pos_cnt'][b] >= 1, (b, facts['pos_cnt'], facts['roi_cnt'])
    assert 0 in facts['proposal_cnt'], 'a sample without proposals: the next one is packed right behind the one before'
    assert facts['empty_grid_balls'] >= 1 and facts['full_grid_balls'] >= 1
    assert facts['seg_classes'] >= 1 and facts['seg_background'] >= 1


@functools.lru_cache(maxsize=None)
def case(variant):
    """-> (inputs, the oracle's outputs, facts); computed once per process and shared: never modify the arrays"""
    if variant == 'truncated':
        case('full')
    inp = make_inputs(SEED, COUNTS, max_out_of(variant))
    out, facts = oracle(inp)
    FACTS[variant] = facts
    _conditions(variant, out, facts)
    return inp, out, facts


REPLAY_COUNTS = (250, 0, 220)               # the graph test's second inputs: other counts, the same total, an empty middle sample


def replay_inputs(variant):
    assert sum(REPLAY_COUNTS) == sum(COUNTS)
    return make_inputs(SEED + 1, REPLAY_COUNTS, max_out_of(variant))


MID_TRUNCATED_BY = 5


@functools.lru_cache(maxsize=None)
def mid_truncation():
    """the committed points with layer 2 — the FIRST strided layer — cut MID_TRUNCATED_BY rows short: the submanifold layer, the last
    strided layer and everything pooled from levels 2 and 3 must see exactly the rows that are left -> (inputs, oracle's A-E, facts)"""
    total2, _ = _totals()
    inp = make_inputs(SEED, COUNTS, (total2 - MID_TRUNCATED_BY, B * 2 * 4 * 4))
    out, facts = oracle(inp, with_roi=False)
    full = case('full')[2]
    lost = [a - b for a, b in zip(full['level_cnt'][1], facts['level_cnt'][1])]
    assert out['B.l1.num'].tolist() == [total2 - MID_TRUNCATED_BY, total2] and lost == [0, 0, MID_TRUNCATED_BY], (out['B.l1.num'], lost)
    assert facts['level_rows'][1] == (total2 - MID_TRUNCATED_BY,) * 2, 'no dead row is left at level 2'
    last, last_full = out[f'B.l{LEVELS[-1][1]}.features'], case('full')[1][f'B.l{LEVELS[-1][1]}.features']
    assert not np.array_equal(last[:facts['level_rows'][2][0]], last_full[:full['level_rows'][2][0]]), 'the cut must reach the last level'
    return inp, out, facts


def isolation_inputs():
    """the 'full' case with the points of sample 0 replaced by another draw of the same count"""
    inp = dict(case('full')[0])
    other, _ = make_points(SEED + 2, COUNTS)
    points = inp['points'].copy()
    points[:COUNTS[0]] = other[:COUNTS[0]]
    assert not np.array_equal(points[:COUNTS[0]], inp['points'][:COUNTS[0]]) and np.array_equal(points[COUNTS[0]:], inp['points'][COUNTS[0]:])
    inp['points'] = points
    return inp


CASES = {variant: case(variant) for variant in VARIANTS}      # built, and their conditions asserted, when the module is imported
