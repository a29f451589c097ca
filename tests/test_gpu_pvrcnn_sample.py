"""PV-RCNN's RoI assign-and-sample stage on the MI355X (csrc/roi_sample.hip): the cases of tests/pvrcnn_sample_ref.py on cuda:0.  The
pairwise IoU within the fp64 bound and bit-identical to the `_cpu` twin; every output of `pvrcnn_assign_and_sample` EQUAL to the
restatement and to the twin in the list, stacked and padded forms — among them the cases that take two and three rounds of the
pair queue, two to four chunks of proposals, every limit at once and pairs on the edges of the cheap overlap tests; device counts
past the limits; every output element written and nothing beyond; hostile values, the same bits as the twin; default keys;
proposals -> sampled RoIs -> targets -> losses -> gradients captured in one graph; and a graph captured on one queue round
replayed on three."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_sample_ref as ref
import pvrcnn_train_ref as train_ref
from mmdet3d_gaussian_amd import _host, _lib, pvrcnn_sample
from test_cpu_pvrcnn_sample import (INT_KEYS, PAD_P, ROW_KEYS, check_clamped, check_default_keys, check_equal, check_hostile, check_iou_values,
                                    run_package, same_bits)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_iou_values_against_fp64_and_the_twin():
    got, hand = check_iou_values(DEV)
    a, b, _, ha, hb, _ = ref.iou_inputs()
    assert torch.equal(got, amd.bbox_overlaps_3d(a, b)) and torch.equal(hand, amd.bbox_overlaps_3d(ha, hb).diagonal())
    assert amd.bbox_overlaps_3d(a[:0].to(DEV), b.to(DEV)).shape == (0, 33)


@pytest.mark.parametrize('name', ref.CASES)
def test_device_equals_the_restatement_and_the_twin(name):
    case, want, _ = ref.reference(name)
    lists = run_package(case, dev=DEV, form='lists')
    check_equal(lists, want)
    twin = run_package(case, dev='cpu', form='lists')
    stacked = run_package(case, dev=DEV, form='stacked')
    again = run_package(case, dev=DEV, form='stacked')
    for k in lists:
        assert torch.equal(lists[k], twin[k]) and torch.equal(lists[k], stacked[k]) and torch.equal(stacked[k], again[k]), k
    check_equal(run_package(case, dev=DEV, form='padded'), want, padded=True)


# 1, 65 and 1025 proposals; three rounds of the pair queue; 4096 proposals on 1024 gts with num = 1024
@pytest.mark.parametrize('name', ['b4_tiny', 'b3_middle_empty', 'b1_1025_65', 'dense_three_rounds', 'limits'])
def test_every_output_element_is_written(name):
    """the C entry point on sentinel-filled outputs with a guard row either side: every row is written — the rows past the counts'
    sums as batch id -1 and zeros, the scratch in full — and nothing beyond the arrays"""
    case, want, _ = ref.reference(name)
    props, gts = torch.cat(case['proposals']).to(DEV), torch.cat(case['gt_bboxes']).to(DEV)
    plab, glab = torch.cat(case['proposal_labels']).to(DEV), torch.cat(case['gt_labels']).to(DEV)
    pc = torch.tensor([p.shape[0] for p in case['proposals']], dtype=torch.int32, device=DEV)
    gc = torch.tensor([g.shape[0] for g in case['gt_bboxes']], dtype=torch.int32, device=DEV)
    keys, fill = case['keys'].to(DEV), case['fill_keys'].to(DEV)
    B, N, G = pc.numel(), props.shape[0], gts.shape[0]
    pos, neg, low, flags = pvrcnn_sample._assigner_rules(case['assigner'])
    num, npos, fracs, thrs = pvrcnn_sample._sampler_rules(case['sampler'])
    host = pvrcnn_sample._host_arrays(pos, neg, low, flags, fracs, thrs)
    S = -77

    def buf(rows, cols=None, dtype=torch.float32):
        return torch.full((rows + 2,) if cols is None else (rows + 2, cols), S, dtype=dtype, device=DEV)
    out = dict(rois=buf(B * num, 8), ious=buf(B * num), inds=buf(B * num, dtype=torch.int64), pos_bboxes=buf(B * npos, 7),
               pos_gt_bboxes=buf(B * npos, 7), pos_assigned_gt_inds=buf(B * npos, dtype=torch.int64), pos_batch_cnt=buf(B, dtype=torch.int32),
               roi_batch_cnt=buf(B, dtype=torch.int32), gt_inds=buf(N, dtype=torch.int64), max_overlaps=buf(N), labels=buf(N, dtype=torch.int64))
    stage = buf(B * (2 + num), dtype=torch.int32)
    p = lambda t: t.data_ptr() if t.numel() else None
    lib = _lib.load()
    _lib.check(lib.gd3d_roi_assign_sample(p(props), p(plab), pc.data_ptr(), N, p(gts), p(glab), gc.data_ptr(), G, B, p(keys), fill.data_ptr(),
                                          len(pos), *host[:4], num, npos, len(thrs), *host[4:],
                                          *(out[k][1:].data_ptr() for k in ('rois', 'ious', 'inds', 'pos_bboxes', 'pos_gt_bboxes',
                                                                            'pos_assigned_gt_inds', 'pos_batch_cnt', 'roi_batch_cnt', 'gt_inds',
                                                                            'max_overlaps', 'labels')),
                                          stage[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), 'gd3d_roi_assign_sample')
    for k, t in out.items():
        assert (t[0] == S).all() and (t[-1] == S).all(), k
        assert torch.equal(t[1:-1].cpu(), want[k]), k
    assert stage[0] == S and stage[-1] == S and not (stage[1:-1] == S).any()
    rows = int(want['roi_batch_cnt'].sum())
    assert (out['rois'][1 + rows:-1, 0] == -1).all() and not out['rois'][1 + rows:-1, 1:].any()


def test_hostile_values_stay_in_bounds():
    """in bounds, and bit for bit what the twin makes of the same hostile values"""
    dev, twin = check_hostile(DEV), check_hostile('cpu')
    for base in dev:
        for k in INT_KEYS + ROW_KEYS:
            assert same_bits(dev[base][k], twin[base][k]), (base, k)


def test_device_counts_past_the_limits_are_clamped():
    dev, twin = check_clamped(DEV), check_clamped('cpu')
    for k in dev:
        assert torch.equal(dev[k], twin[k]), k


def test_default_keys_follow_the_seed():
    check_default_keys(DEV)


def _stacked(case, pad=PAD_P):
    g = torch.Generator().manual_seed(3)
    props = torch.cat(case['proposals'] + [torch.rand(pad, 7, generator=g) + 0.5]).to(DEV)
    plab = torch.cat(case['proposal_labels'] + [torch.zeros(pad, dtype=torch.int64)]).to(DEV)
    keys = torch.cat([case['keys'], torch.rand(pad, generator=g)]).to(DEV)
    pc = torch.tensor([p.shape[0] for p in case['proposals']], dtype=torch.int32, device=DEV)
    gc = torch.tensor([x.shape[0] for x in case['gt_bboxes']], dtype=torch.int32, device=DEV)
    return props, plab, torch.cat(case['gt_bboxes']).to(DEV), torch.cat(case['gt_labels']).to(DEV), pc, gc, keys, case['fill_keys'].to(DEV)


def test_whole_chain_under_graph_capture():
    """proposals -> sampled RoIs -> targets -> losses -> gradients with device counts and keys in static buffers, captured in one
    graph, replayed once on new proposals, counts and keys, and compared with the eager result bit for bit; the RoI rows past the
    counts (batch id -1: the middle sample is empty) contribute nothing to the losses"""
    case, want, _ = ref.reference('b3_middle_empty')
    props, plab, gts, glab, pc, gc, keys, fill = _stacked(case)
    num, B = case['sampler']['num'], 3
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B * num, 1, generator=g).to(DEV).requires_grad_(True)
    p = (0.1 * torch.randn(B * num, 7, generator=g)).to(DEV).requires_grad_(True)
    unit = _host.unit_grad(torch.device(DEV))

    def step():
        s = amd.pvrcnn_assign_and_sample(props, plab, gts, glab, case['assigner'], case['sampler'], prop_batch_cnt=pc, gt_batch_cnt=gc,
                                         keys=keys, fill_keys=fill)
        tg = amd.pvrcnn_head_get_targets(s['pos_bboxes'], s['pos_gt_bboxes'], s['ious'], train_ref.CFG, pos_batch_cnt=s['pos_batch_cnt'],
                                         roi_batch_cnt=s['roi_batch_cnt'])
        losses = amd.pvrcnn_head_loss(train_ref.LOSS_CLS, train_ref.LOSS_BBOX, x, p, s['rois'], *tg)
        vals = [losses[k] for k in train_ref.LOSS_KEYS]
        gx, gp = torch.autograd.grad(vals, [x, p], grad_outputs=[unit] * 3)
        return [s[k] for k in ('rois', 'ious', 'inds', 'pos_bboxes', 'pos_gt_bboxes', 'pos_assigned_gt_inds', 'pos_batch_cnt', 'roi_batch_cnt')] + \
            list(tg) + vals + [gx, gp]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.detach().clone() for t in step()]      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(first[0].cpu(), want['rois']) and torch.equal(first[7].cpu(), want['roi_batch_cnt'])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():                                 # new values in the static buffers: proposals, counts and keys
        props[:, 2].add_(0.05)
        props[:, :2].add_(0.01)
        pc.copy_(torch.tensor([60, 0, 63], dtype=torch.int32))
        keys.copy_(torch.rand(keys.shape, generator=g).to(DEV))
        fill.copy_(torch.rand(fill.shape, generator=g).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[0], first[0]) and not torch.equal(eager[2], first[2]) and not torch.equal(eager[-1], first[-1])
    for got, exp in zip(captured, eager):
        assert torch.equal(got.detach(), exp.detach())
    # the padded rows: no label weight, no box weight, zero gradients; the losses are those of the covered rows alone
    rows, pos = int(eager[7].sum()), int(eager[6].sum())
    assert 0 < rows < B * num and (eager[0][rows:, 0] == -1).all()
    assert not eager[-2][rows:].any() and not eager[-1][rows:].any() and not eager[11][rows:].any() and not eager[12][rows:].any() \
        and not eager[13][rows:].any()
    tg = amd.pvrcnn_head_get_targets(eager[3][:pos], eager[4][:pos], eager[1][:rows], train_ref.CFG, pos_batch_cnt=eager[6], roi_batch_cnt=eager[7])
    alone = amd.pvrcnn_head_loss(train_ref.LOSS_CLS, train_ref.LOSS_BBOX, x[:rows], p[:rows], eager[0][:rows], *tg)
    for k, v in zip(train_ref.LOSS_KEYS, eager[14:17]):
        assert torch.allclose(alone[k], v, rtol=1e-5, atol=1e-7), k


def test_graph_replay_into_more_queue_rounds():
    """static buffers of the size of `dense_three_rounds`, captured while they hold a sparse sample (300 proposals on 5 gts: one
    round of the pair queue), replayed after the dense proposals, gts, counts and keys are copied in (three rounds): the round count
    is data the kernel reads, not something the capture froze.  The replay equals the eager call and the restatement bit for bit."""
    case, want, _ = ref.reference('dense_three_rounds')
    sparse = ref.make_sample(60, ref.mixed(300), 5, C=1)
    assert max(ref.queued_pairs(sparse, 3)) < ref.WL_CAP
    n, g = case['proposals'][0].shape[0], case['gt_bboxes'][0].shape[0]
    props, plab = torch.zeros(n, 7, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    gts, glab = torch.zeros(g, 7, device=DEV), torch.zeros(g, dtype=torch.int64, device=DEV)
    props[:300], plab[:300], gts[:5], glab[:5] = (t.to(DEV) for t in sparse)
    pc, gc = torch.tensor([300], dtype=torch.int32, device=DEV), torch.tensor([5], dtype=torch.int32, device=DEV)
    keys, fill = case['keys'].to(DEV).flip(0), case['fill_keys'].to(DEV).flip(0)
    names = INT_KEYS + ROW_KEYS

    def step():
        out = amd.pvrcnn_assign_and_sample(props, plab, gts, glab, case['assigner'], case['sampler'], prop_batch_cnt=pc, gt_batch_cnt=gc,
                                           keys=keys, fill_keys=fill, return_assignment=True)
        return [out[k] for k in names]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.clone() for t in step()]                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    props.copy_(case['proposals'][0])
    plab.copy_(case['proposal_labels'][0])
    gts.copy_(case['gt_bboxes'][0])
    glab.copy_(case['gt_labels'][0])
    pc.fill_(n)
    gc.fill_(g)
    keys.copy_(case['keys'])
    fill.copy_(case['fill_keys'])
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert int(first[names.index('roi_batch_cnt')][0]) > 0 and not torch.equal(first[names.index('inds')], eager[names.index('inds')])
    for k, got, exp in zip(names, captured, eager):
        assert torch.equal(got, exp) and torch.equal(got.cpu(), want[k]), k


def test_roi_grid_queries_on_the_padded_rows():
    """what `roi_grid_queries` makes of the rows past the counts: batch id -1 belongs to no sample, so the counts it returns cover the
    real RoIs only, and since those rows come LAST their grid points (of a zero box: all zero) lie past the counts' sum, where the
    stacked query ops do not look.  Nothing needs to be dropped."""
    case, want, _ = ref.reference('b3_middle_empty')
    out = run_package(case, dev=DEV, form='stacked')
    rois = out['rois'].to(DEV)
    new_xyz, cnt = amd.roi_grid_queries(rois, 3, grid_size=6)
    rows = int(want['roi_batch_cnt'].sum())
    assert rows < rois.shape[0] and torch.equal(cnt.cpu(), want['roi_batch_cnt'] * 216)
    assert new_xyz.shape == (rois.shape[0] * 216, 3) and not new_xyz[rows * 216:].any() and torch.isfinite(new_xyz).all()
