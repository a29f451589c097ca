"""PV-RCNN's RPN proposal stage on the MI355X (csrc/rpn_proposal.hip): every case of tests/rpn_proposal_ref.py on cuda:0 EQUAL to the
`_cpu` twin on every output; the boundaries of the launches' own tiling (the histogram span, the ordering launch's group and tile, the streaming
launch's workgroup of cells, W = 1, the boundary key's holders spread over several spans); one selection of 9000 from 10 560
anchors against numpy's stable argsort and against the package's existing NMS driven from torch; refused maps; capture on one
stream with `pvrcnn_assign_and_sample` behind it in the same graph; two eager runs with equal bits."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_sample_ref as sref
import rpn_proposal_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPAN, TILE, RANK, CELLS = 4096, 256, 64, 256      # csrc/rpn_proposal_common.h: SPAN keys a histogram workgroup; the ordering launch's
#                                                   LDS tile and the RANK_I survivors a workgroup ranks; WG cells a streaming workgroup


def t(a, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(c, dev, **kw):
    out = amd.rpn_proposals(t(c['cls'], dev), t(c['bbox'], dev), t(c['dirp'], dev), t(c['anchors'], dev), c['cfg'], c['C'],
                            dir_offset=c.get('dir_offset', 0.7854), dir_limit_offset=c.get('dir_limit_offset', 0.0), return_candidates=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('name', sorted(ref.BUILDERS))
def test_device_equals_the_twin(name):
    got = ref.run_case(amd, name, DEV)
    ref.same(got, ref.run_case(amd, name, 'cpu'), name)
    ref.same(got, ref.case_expected(name), name)


def _shape_case(seed, H, W, A, C, nms_pre, **cfg):
    c = ref.make_inputs(seed, 2, H, W, A, C)
    c.update(cfg=ref.cfg_of(nms_pre, **cfg))
    return c


BOUNDARIES = {
    # the histogram / compaction workgroup's span of SPAN = 4096 keys (A = 1: anchors = cells)
    'span_minus_1': lambda: _shape_case(40, 5, 819, 1, 2, 300),          # 4095
    'span': lambda: _shape_case(41, 64, 64, 1, 2, 300),                   # 4096
    'span_plus_1': lambda: _shape_case(42, 17, 241, 1, 2, 300),           # 4097
    # the ordering launch: 64 survivors a workgroup, tiles of 256 survivors through LDS
    'rank_minus_1': lambda: _shape_case(37, 5, 7, 6, 3, RANK - 1),
    'rank': lambda: _shape_case(38, 5, 7, 6, 3, RANK),
    'rank_plus_1': lambda: _shape_case(39, 5, 7, 6, 3, RANK + 1),
    'tile_minus_1': lambda: _shape_case(43, 8, 11, 6, 3, TILE - 1),
    'tile': lambda: _shape_case(44, 8, 11, 6, 3, TILE),
    'tile_plus_1': lambda: _shape_case(45, 8, 11, 6, 3, TILE + 1),
    # the streaming launch reads scalar words along the flattened (h, w) of a plane — its "vector" is one word, so no W is special
    # but for the workgroup's 256 cells: 255, 256, 257 cells, the last as W = 1; W = 7 and 11 (odd) run in the named cases
    'cells_minus_1': lambda: _shape_case(46, 5, 51, 2, 3, 200),
    'cells': lambda: _shape_case(47, 16, 16, 2, 3, 200),
    'cells_plus_1_W1': lambda: _shape_case(48, 257, 1, 2, 3, 200),
}


@pytest.mark.parametrize('name', sorted(BOUNDARIES))
def test_tiling_boundaries_equal_the_twin(name):
    c = BOUNDARIES[name]()
    N = c['cls'].shape[2] * c['cls'].shape[3] * (c['cls'].shape[1] // c['C'])
    assert {'span': N - SPAN, 'tile': c['cfg']['nms_pre'] - TILE, 'rank': c['cfg']['nms_pre'] - RANK, 'cell': c['cls'].shape[2] * c['cls'].shape[3] - CELLS}[name[:4]] == \
        (-1 if 'minus' in name else 1 if 'plus' in name else 0)
    ref.same(run(c, DEV), run(c, 'cpu'), name)


def test_boundary_key_holders_spread_over_several_spans():
    """logits rounded to one decimal: masses of equal keys in three spans and a remainder; the boundary key's holders are taken by
    ascending index across the spans (the span counts' sum), which the order itself shows: equal to numpy's stable argsort"""
    c = _shape_case(49, 1, 3 * SPAN + 5, 1, 2, 500, nms_thr=0.3)
    c['cls'] = np.round(c['cls'], 1).astype(np.float32)
    got = run(c, DEV)
    L = ref.anchor_rows(c['cls'], 2)
    for b in range(2):
        sel, best, _ = ref.select(L[b], 500)
        assert np.array_equal(got['cand_inds'][b], sel)
        holders = np.nonzero(L[b].max(1) == best[-1])[0]
        taken = np.intersect1d(holders, sel)
        assert len(holders) > len(taken) > 0 and holders[-1] >= 2 * SPAN and np.array_equal(taken, holders[:len(taken)])
    ref.same(got, run(c, 'cpu'), 'ties over spans')


def test_large_selection_against_argsort_and_the_existing_nms_path():
    """nms_pre = 9000 of 40 x 44 x 6 = 10 560 anchors, B = 2: the selected anchors and their order against numpy's stable argsort; the
    final outputs against the restatement whose NMS step is the package's existing `nms_gpu` on the device, driven from torch on the
    same candidates (the CPU NMS twin is not run at this size)."""
    c = ref.make_inputs(50, 2, 40, 44, 6, 3)
    c.update(cfg=ref.cfg_of(9000, 512, 512, nms_thr=0.8, score_thr=0.3))
    got = run(c, DEV)
    L = ref.anchor_rows(c['cls'], 3)
    for b in range(2):
        best = L[b].max(1)
        order = np.argsort(-ref.key_of(best).astype(np.int64), kind='stable')[:9000]
        assert np.array_equal(got['cand_inds'][b], order)

    def device_nms(bev, thr, rotate):
        assert rotate
        scores = torch.arange(len(bev), 0, -1, dtype=torch.float32, device=DEV)      # the rows are in the selection order already
        return amd.nms_gpu_batched(t(bev), scores[None], thr)[0].cpu().numpy()
    want = ref.expected(c['cls'], c['bbox'], c['dirp'], c['anchors'], c['cfg'], 3, nms=device_nms)
    assert want['batch_cnt'].min() > 100 and want['cand_cnt'].min() > 5000
    ref.same(got, want, 'large')


def test_refused_maps_launch_nothing():
    c = ref.case('pre_N')
    cls, bbox, dirp, an = t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors'])
    with pytest.raises(RuntimeError, match='fp32'):
        amd.rpn_proposals(cls.half(), bbox, dirp, an, c['cfg'], 3)
    with pytest.raises(RuntimeError, match='fp32'):
        amd.rpn_proposals(cls, bbox, dirp.double(), an, c['cfg'], 3)
    with pytest.raises(RuntimeError, match='contiguous'):
        amd.rpn_proposals(cls, bbox.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), dirp, an, c['cfg'], 3)
    with pytest.raises(RuntimeError, match='contiguous'):
        amd.rpn_proposals(cls.repeat(1, 1, 1, 2)[..., ::2], bbox, dirp, an, c['cfg'], 3)
    with pytest.raises(RuntimeError, match='is on'):
        amd.rpn_proposals(cls, bbox.cpu(), dirp, an, c['cfg'], 3)
    torch.cuda.synchronize()


def test_two_eager_runs_give_equal_bits():
    c = ref.make_inputs(51, 2, 40, 44, 6, 3)
    c.update(cfg=ref.cfg_of(2000, 200, 300, nms_thr=0.7))
    a, b = run(c, DEV), run(c, DEV)
    ref.same(a, b, 'rerun')


def test_capture_on_one_stream_with_assign_and_sample_behind():
    """the call captured on one stream with `pvrcnn_assign_and_sample` fed by its boxes_3d / labels_3d / batch_cnt inside the same
    graph; replayed on fresh head maps and compared with the eager calls bit for bit"""
    c, fresh = ref.make_inputs(52, 3, 8, 11, 6, 3), ref.make_inputs(53, 3, 8, 11, 6, 3)
    fresh['cls'][1] = -2.0 - np.abs(fresh['cls'][1])          # the replay meets an empty sample the capture did not
    cfg = ref.cfg_of(300, 40, 50)
    cls, bbox, dirp, an = t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors'])
    g = torch.Generator().manual_seed(4)
    gts = (torch.rand(9, 7, generator=g) * torch.tensor([8.0, 6.0, 0.5, 1.0, 2.0, 0.5, 3.0]) + torch.tensor([0.0, -3.0, -1.8, 1.0, 2.0, 1.3, 0.0])).to(DEV)
    glab = torch.randint(0, 3, (9,), generator=g).to(DEV)
    gcnt = torch.tensor([3, 3, 3], dtype=torch.int32, device=DEV)
    keys, fill = torch.rand(3 * 40, generator=g).to(DEV), torch.rand(3 * 16, generator=g).to(DEV)
    sampler = sref._sampler(16)
    names = ('boxes_3d', 'scores_3d', 'labels_3d', 'cls_preds', 'rois', 'batch_cnt')

    def step():
        p = amd.rpn_proposals(cls, bbox, dirp, an, cfg, 3)
        s = amd.pvrcnn_assign_and_sample(p['boxes_3d'], p['labels_3d'], gts, glab, sref.RPN_STYLE, sampler, prop_batch_cnt=p['batch_cnt'],
                                         gt_batch_cnt=gcnt, keys=keys, fill_keys=fill)
        return [p[k] for k in names] + [s['rois'], s['inds'], s['roi_batch_cnt']]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [x.clone() for x in step()]                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    cls.copy_(t(fresh['cls']))
    bbox.copy_(t(fresh['bbox']))
    dirp.copy_(t(fresh['dirp']))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[0], first[0]) and eager[5].tolist()[1] == 0 and int(eager[-1].sum()) > 0
    for got, exp in zip(captured, eager):
        assert torch.equal(got, exp)
    fresh.update(cfg=cfg)
    twin = run(fresh, 'cpu')
    for k, got in zip(names, captured):
        assert np.array_equal(got.cpu().numpy().view(np.uint8), twin[k].view(np.uint8)), k
