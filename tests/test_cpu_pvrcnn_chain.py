"""PV-RCNN's op hand-offs end to end through the `_cpu` twins: hard_voxelize -> four sparse layers -> voxel_centers / sample_keypoints ->
QueryAndGroup and VoxelQueryAndGroup per level -> dense() -> bev_interpolate, and rpn_proposals -> pvrcnn_assign_and_sample ->
roi_grid_queries -> QueryAndGroup, each op fed by the one before it in its static form, against the chained oracle of
tests/pvrcnn_chain_ref.py (stage k of the oracle consumes the oracle's stage k - 1, never a product output).

  * every stage boundary EQUAL to the oracle (values; a signed zero is a zero), dead rows included; the bilinear sum of
    `bev_interpolate` within the bound of its own suite (vsa_bev_ref.check_values, unchanged) — printed per tensor;
  * the rows of samples 1 and 2 keep their values when the points of sample 0 are replaced;
  * a negative control: the wrong `scale_factor` handed to `voxel_query_coords` at level 2 IS seen, and only there;
  * other per-sample counts with a sample WITHOUT points: equal to the oracle, that sample's keypoints finding empty balls;
  * the first strided layer cut short by `max_out`, mid-chain: every later stage sees exactly the rows that are left.
The checks take a device: tests/test_gpu_pvrcnn_chain.py runs them on cuda:0.

What the committed seeds give (pvrcnn_chain_ref.FACTS, asserted there): see DESIGN.md §4."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_chain_ref as ref
import vsa_bev_ref as vb

PREFIX_KEYS = ('F.sample.gt_inds', 'F.sample.max_overlaps', 'F.sample.labels')      # one entry per proposal the counts cover


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Chain:
    """The product chain on `dev` over static input buffers (`load` refills them in place: the graph test replays on them).
    `run` -> {key: tensor} under the oracle's keys; `layout[key]` = (the key of the per-sample row counts the tensor is stacked by, or
    None where dimension 0 is the sample; the key of the counts whose row offsets its VALUES carry, or None)."""

    def __init__(self, inp, dev, with_roi=True):
        self.dev, self.with_roi, self.layout = dev, with_roi, {}
        self.points, self.cnt = t(inp['points'], dev), t(inp['cnt'], dev)
        self.layers = []
        for i, (subm, W) in enumerate(zip(ref.LAYERS, inp['weights'])):
            cin, cout = W.shape[1:]
            layer = (amd.SubMConv3d(cin, cout, 3, bias=False, indice_key=f'l{i}') if subm else
                     amd.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=False, indice_key=f'l{i}', max_out=inp['max_out'][i // 2]))
            with torch.no_grad():
                layer.weight.copy_(t(W, 'cpu').reshape(layer.weight.shape))
            self.layers.append(layer.to(dev).requires_grad_(False))
        if with_roi:
            c = ref.roi_inputs()
            self.head = [t(c[k], dev) for k in ('cls', 'bbox', 'dirp', 'anchors')]
            self.gts, self.glab = [t(g, dev) for g in c['gts']], [t(g, dev) for g in c['glab']]
            self.gcnt = torch.tensor([len(g) for g in c['gts']], dtype=torch.int32).to(dev)
            self.keys, self.fill = t(c['keys'], dev), t(c['fill_keys'], dev)

    def load(self, inp):
        self.points.copy_(t(inp['points'], self.dev))
        self.cnt.copy_(t(inp['cnt'], self.dev))

    @torch.no_grad()
    def run(self, coords_scale=None):
        out, B, K = {}, ref.B, ref.K
        vs, rng = ref.VOXEL_SIZE, ref.RANGE

        def put(key, value, rows=None, base=None):
            out[key], self.layout[key] = value, (rows, base)

        # A: the static voxelizer
        voxels, coors, num_points, vcnt, mean = amd.hard_voxelize(self.points, vs, rng, ref.P, ref.MV, points_batch_cnt=self.cnt, with_mean=True,
                                                                  static=True)
        put('A.voxel_batch_cnt', vcnt)
        for k, v in (('voxels', voxels), ('coors', coors), ('num_points', num_points), ('mean', mean)):
            put(f'A.{k}', v, 'A.voxel_batch_cnt')
        # B: integer features from the voxelizer's own outputs, zero on dead rows; four layers, ReLU after each
        feats = torch.cat([num_points[:, None], coors[:, 1:]], 1).float()
        feats = torch.where((num_points > 0)[:, None], feats, torch.zeros_like(feats))
        put('B.in', feats, 'A.voxel_batch_cnt')
        x = amd.SparseConvTensor(feats, coors, ref.SHAPE, B)
        levels = []
        for i, layer in enumerate(self.layers):
            x = layer(x)
            x.features = torch.relu(x.features)
            index = x.indice_dict[f'l{i}']
            put(f'B.l{i}.cnt', index.out_batch_cnt)
            put(f'B.l{i}.indices', x.indices, f'B.l{i}.cnt')
            put(f'B.l{i}.features', x.features, f'B.l{i}.cnt')
            if not layer.subm:
                put(f'B.l{i}.num', index.num[None])           # (1, 2): kept and true row counts of the whole batch
            levels.append(x)
        # C: keypoints from the raw points and from the voxel centres
        xyz1, cnt1 = amd.voxel_centers(coors, vs, rng, 1, 'half', B)
        kps = dict(raw=amd.sample_keypoints(self.points[:, :3], self.cnt, K), vox=amd.sample_keypoints(xyz1, cnt1, K))
        key_cnt = torch.full((B,), K, dtype=torch.int32, device=self.dev)
        put('C.key_cnt', key_cnt)
        put('C.raw.kp', kps['raw'])
        put('C.vox.kp', kps['vox'])
        put('C.vox.cnt', cnt1)
        put('C.vox.xyz', xyz1, 'C.vox.cnt')
        # D: per level, the ball query and the voxel query over the level's rows; E: the last level as the BEV map
        last = levels[ref.LEVELS[-1][1]]
        bev = last.dense().view(B, -1, last.spatial_shape[1], last.spatial_shape[2])
        put('E.bev', bev)
        for align in ref.ALIGNS:
            for n, (stride, li) in enumerate(ref.LEVELS):
                lv, name = levels[li], ref.level_name(stride)
                xyz, xcnt = amd.voxel_centers(lv.indices, vs, rng, stride, align, B)
                f = torch.cat([lv.features, mean], 1) if stride == 1 else lv.features
                index = amd.voxel_query_index(lv.indices, lv.spatial_shape, B)
                cnt_key = f'D.{align}.{name}.cnt'
                put(cnt_key, xcnt)
                put(f'D.{align}.{name}.xyz', xyz, cnt_key)
                put(f'D.{name}.skey', index.skey, cnt_key)
                put(f'D.{name}.srow', index.srow, cnt_key, cnt_key)
                ball = amd.QueryAndGroup(ref.RADIUS[n], ref.NSAMPLE)
                voxel = amd.VoxelQueryAndGroup(ref.MAX_RANGE[n], ref.RADIUS[n], ref.NSAMPLE)
                for src in ref.SOURCES:
                    q, tag = kps[src].reshape(-1, 3), f'D.{src}.{align}.{name}'
                    g, idx = ball(xyz, xcnt, q, key_cnt, f)
                    scale = stride if coords_scale is None else coords_scale.get(stride, stride)
                    nc = amd.voxel_query_coords(q, key_cnt, vs, rng, scale)
                    vg, vidx = voxel(xyz, q, nc, index, f)
                    put(f'{tag}.ball.out', g, 'C.key_cnt')
                    put(f'{tag}.ball.idx', idx, 'C.key_cnt')
                    put(f'{tag}.ball.pooled', g.max(-1).values, 'C.key_cnt')
                    put(f'{tag}.voxel.coords', nc, 'C.key_cnt')
                    put(f'{tag}.voxel.out', vg, 'C.key_cnt')
                    put(f'{tag}.voxel.idx', vidx, 'C.key_cnt', cnt_key)
                    put(f'{tag}.voxel.pooled', vg.max(-1).values, 'C.key_cnt')
        for src in ref.SOURCES:
            for align in ref.ALIGNS:
                put(f'E.{src}.{align}.interp', amd.bev_interpolate(kps[src], bev, vs, rng, ref.LEVELS[-1][0], align))
        if self.with_roi:
            self.roi_side(put, out, kps, key_cnt)
        return out

    def roi_side(self, put, out, kps, key_cnt):
        """F: proposals -> assign-and-sample -> RoI grid queries -> QueryAndGroup over the keypoints with D's pooled features"""
        B, C = ref.B, ref.HEAD['C']
        p = amd.rpn_proposals(*self.head, ref.RPN_CFG, C)
        put('F.prop.batch_cnt', p['batch_cnt'])
        for k in ('boxes_3d', 'scores_3d', 'labels_3d', 'cls_preds', 'rois'):
            put(f'F.prop.{k}', p[k], 'F.prop.batch_cnt')
        s = amd.pvrcnn_assign_and_sample(p['boxes_3d'], p['labels_3d'], torch.cat(self.gts), torch.cat(self.glab), ref.ASSIGNER, ref.SAMPLER,
                                         prop_batch_cnt=p['batch_cnt'], gt_batch_cnt=self.gcnt, keys=self.keys, fill_keys=self.fill,
                                         return_assignment=True)
        put('F.sample.roi_batch_cnt', s['roi_batch_cnt'])
        put('F.sample.pos_batch_cnt', s['pos_batch_cnt'])
        for k in ('rois', 'ious', 'inds'):
            put(f'F.sample.{k}', s[k], 'F.sample.roi_batch_cnt')
        for k in ('pos_bboxes', 'pos_gt_bboxes', 'pos_assigned_gt_inds'):
            put(f'F.sample.{k}', s[k], 'F.sample.pos_batch_cnt')
        for k in ('gt_inds', 'max_overlaps', 'labels'):
            put(f'F.sample.{k}', s[k], 'F.prop.batch_cnt')
        grid, grid_cnt = amd.roi_grid_queries(s['rois'], B, ref.GRID)
        put('F.grid_cnt', grid_cnt)
        put('F.grid', grid, 'F.grid_cnt')
        src, align, stride = ref.ROI_FEATURES
        flat = kps[src].reshape(-1, 3)
        g, idx = amd.QueryAndGroup(ref.ROI_RADIUS, ref.ROI_NSAMPLE)(flat, key_cnt, grid, grid_cnt, out[f'D.{src}.{align}.{ref.level_name(stride)}.ball.pooled'])
        put('F.ball.out', g, 'F.grid_cnt')
        put('F.ball.idx', idx, 'F.grid_cnt')
        ids = torch.arange(B, device=self.dev, dtype=torch.float32).repeat_interleave(ref.K)[:, None]
        seg, box_idx = amd.pointwise_mask_targets(torch.cat([ids, flat], 1), None, self.gts, self.glab, ref.EXTRA_WIDTH, C, return_box_idx=True)
        put('F.seg', seg, 'C.key_cnt')
        put('F.box_idx', box_idx, 'C.key_cnt')


def run_chain(dev, inp, with_roi=True, coords_scale=None):
    """-> ({key: CPU tensor}, layout)"""
    chain = Chain(inp, dev, with_roi)
    out = chain.run(coords_scale)
    return {k: v.cpu() for k, v in out.items()}, chain.layout


def same(a, b):
    """equal dtype, shape and values, nothing NaN (a signed zero is a zero)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and not (a.dtype.kind == 'f' and np.isnan(a).any()) and bool(np.array_equal(a, b))


def differing_keys(got, want, what):
    """the keys of the oracle's dict `want` on which `got` (CPU tensors) is not EQUAL to it; the interpolated features are held to the
    bound of `bev_interpolate`'s own suite instead (figures printed) and listed when they miss it"""
    bad = []
    for k, w in want.items():
        g = got[k]
        if k.endswith('.interp'):
            try:
                vb.check_values(dict(out=g), dict(out=w[0]), dict(out=w[1]), ('out',), f'{what} {k}')
            except AssertionError as e:
                bad.append((k, str(e)))
            continue
        g = g.numpy()
        if k in PREFIX_KEYS:
            assert len(g) >= len(w), k
            g = g[:len(w)]
        if k.endswith('.num'):
            g = g[0]
        if not same(g, w):
            where = np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else (g.shape, w.shape)
            bad.append((k, g.dtype, w.dtype, where))
    return bad


def _offsets(cnt):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt.long(), 0)])


def check_dead_rows(got):
    """the static forms end in dead rows — coors -1, zero features — that no count includes and no index names; levels stay grouped by
    ascending sample"""
    V = int(got['A.voxel_batch_cnt'].sum())
    assert V < len(got['A.coors']) and (got['A.coors'][V:] == -1).all() and (got['A.coors'][:V] >= 0).all()
    assert not got['A.num_points'][V:].any() and (got['A.num_points'][:V] > 0).all()
    assert not got['A.voxels'][V:].any() and not got['A.mean'][V:].any() and not got['B.in'][V:].any()
    for i in range(len(ref.LAYERS)):
        ind, feats, cnt = got[f'B.l{i}.indices'], got[f'B.l{i}.features'], got[f'B.l{i}.cnt']
        kept = int(cnt.sum())
        assert (ind[kept:] == -1).all() and (ind[:kept] >= 0).all() and not feats[kept:].any()
        assert (ind[1:kept, 0] >= ind[:kept - 1, 0]).all(), 'grouped by ascending sample'
        assert torch.equal(torch.bincount(ind[:kept, 0].long(), minlength=ref.B).int(), cnt)
    sample = torch.arange(ref.B).repeat_interleave(ref.K)
    for align in ref.ALIGNS:
        for stride, li in ref.LEVELS:
            name = ref.level_name(stride)
            cnt, ind = got[f'D.{align}.{name}.cnt'], got[f'B.l{li}.indices']
            assert torch.equal(cnt, got[f'B.l{li}.cnt']), 'voxel_centers counts what the layer kept'
            kept = int(cnt.sum())
            srow = got[f'D.{name}.srow'].long()
            assert (ind[srow[:kept], 0] >= 0).all() and (ind[srow[kept:], 0] == -1).all(), 'the dead rows sort last'
            for src in ref.SOURCES:
                tag = f'D.{src}.{align}.{name}'
                idx, vidx = got[f'{tag}.ball.idx'].long(), got[f'{tag}.voxel.idx'].long()
                assert (idx >= 0).all() and (idx < cnt[sample].clamp(min=1)[:, None]).all(), 'a ball names rows of its own sample only'
                assert ((ind[vidx, 0] == sample[:, None]) | (vidx == 0)).all(), 'a voxel query names live rows of its own sample only'


def check_chain(dev, variant):
    """every stage boundary of the product chain on `dev` against the chained oracle"""
    inp, want, facts = ref.case(variant)
    print(f'{variant}: {facts}')
    got, _ = run_chain(dev, inp)
    assert set(want) <= set(got)
    bad = differing_keys(got, want, f'{dev} {variant}')
    assert not bad, bad
    check_dead_rows(got)
    return got


def check_sample_isolation(dev):
    """sample 0's points replaced by another draw of the same count: every stage output keeps the values of samples 1 and 2 — stacked
    outputs through the per-sample counts, row indices after subtracting the sample's row offset"""
    inp = ref.case('full')[0]
    a, layout = run_chain(dev, inp)
    b, _ = run_chain(dev, ref.isolation_inputs())
    assert not torch.equal(a['A.coors'], b['A.coors']) and not torch.equal(a['C.raw.kp'][0], b['C.raw.kp'][0])
    for i in (1, 3):
        assert int(b[f'B.l{i}.num'][0, 1]) <= len(b[f'B.l{i}.indices']), 'the other draw must not truncate a level'
    moved = 0
    for key, (rows, base) in layout.items():
        if key.endswith('.num'):            # the whole batch's row counts: sample 0's are in them
            continue
        if rows is None:
            assert a[key].size(0) == ref.B, key
            assert torch.equal(a[key][1:], b[key][1:]), key
            continue
        ca, cb = a[rows], b[rows]
        assert torch.equal(ca[1:], cb[1:]), (key, rows)
        oa, ob = _offsets(ca), _offsets(cb)
        for s in (1, 2):
            va, vb_ = a[key][oa[s]:oa[s + 1]], b[key][ob[s]:ob[s + 1]]
            if base is not None:            # global rows of the level: local to the sample, 0 staying the empty query's 0
                ba, bb = _offsets(a[base]), _offsets(b[base])
                moved += int(ba[s] != bb[s])
                va = torch.where(va == 0, va, va - ba[s].to(va.dtype))
                vb_ = torch.where(vb_ == 0, vb_, vb_ - bb[s].to(vb_.dtype))
            assert torch.equal(va, vb_), (key, s)
    assert moved > 0, 'no level moved its rows: the offsets were not under test'


def check_stride_mismatch_is_visible(dev):
    """the negative control of the comparison itself: `voxel_query_coords` handed scale_factor 1 where level 2 has stride 2 — the
    product chain then differs from the oracle, on that level's voxel-query outputs and nowhere else"""
    inp, want, _ = ref.case('full')
    got, _ = run_chain(dev, inp, coords_scale={2: 1})
    bad = {entry[0] for entry in differing_keys(got, want, f'{dev} stride mismatch')}
    assert bad, 'a scale slip went unseen'
    assert all('.s2.voxel.' in k for k in bad), sorted(bad)
    assert any(k.endswith('.voxel.coords') for k in bad) and any(k.endswith('.voxel.pooled') for k in bad), sorted(bad)


def points_side(want):
    """the oracle's stages A-E"""
    return {k: v for k, v in want.items() if not k.startswith('F.')}


def check_empty_sample(dev, variant='truncated', got=None):
    """other per-sample counts with NO point in sample 1 (the graph test's second inputs), stages A-E: equal to the oracle on those inputs;
    sample 1 has no voxel at any level, so its keypoints — rows clamped into the array, another sample's points — find empty balls and
    a zero BEV row, not the rows of the sample they were taken from"""
    inp = ref.replay_inputs(variant)
    want, facts = ref.oracle(inp, with_roi=False)
    assert inp['cnt'].tolist() == list(ref.REPLAY_COUNTS) and inp['cnt'][1] == 0 and facts['level_cnt'][0][1] == 0
    if got is None:
        got, _ = run_chain(dev, inp, with_roi=False)
    bad = differing_keys(got, want, f'{dev} empty middle sample')
    assert not bad, bad
    K = ref.K
    assert torch.equal(got['C.raw.kp'][1], got['C.raw.kp'][2][:1].expand(K, 3)), 'the clamped row: the first point of sample 2'
    for key, value in got.items():
        if key.endswith('.pooled') or key.endswith('.interp'):
            rows = value.reshape(ref.B, K, -1)
            assert not rows[1].any() and rows[0].any() and rows[2].any(), key
    return facts


def check_mid_chain_truncation(dev):
    """the first strided layer cut short by its `max_out`: every later stage equals the oracle on the rows that are left"""
    inp, want, _ = ref.mid_truncation()
    got, _ = run_chain(dev, inp, with_roi=False)
    bad = differing_keys(got, want, f'{dev} layer 2 truncated')
    assert not bad, bad
    kept = int(got['B.l1.cnt'].sum())
    assert kept == len(got['B.l1.indices']) and (got['B.l1.indices'] >= 0).all()


@pytest.mark.parametrize('variant', ref.VARIANTS)
def test_the_case_keeps_its_conditions(variant):
    """empty and crowded balls at every level, ball query and voxel query agreeing and differing, the wrap-around, dead tail rows, the
    cut by max_voxels, the truncated cells, pad rows, positives and negatives, empty RoI grid balls: asserted by the builder"""
    _, _, facts = ref.case(variant)
    assert facts is ref.FACTS[variant]
    print(variant, facts)


@pytest.mark.parametrize('variant', ref.VARIANTS)
def test_every_stage_boundary_equals_the_chained_oracle(variant):
    check_chain('cpu', variant)


def test_samples_do_not_leak_into_each_other():
    check_sample_isolation('cpu')


def test_a_stride_mismatch_is_visible():
    check_stride_mismatch_is_visible('cpu')


def test_an_empty_sample_finds_empty_balls():
    check_empty_sample('cpu')


def test_a_level_truncated_mid_chain_is_seen_downstream():
    check_mid_chain_truncation('cpu')
