"""PVRCNNBboxHead's training slice on the MI355X (csrc/roi_head.hip): the shapes and seeds of tests/test_cpu_pvrcnn_train.py on cuda:0.
Decisions bit-identical to the `_cpu` twin and to the fp32 restatement, values and gradients within the same bounds against the fp64
restatement (computed on the CPU, once per case), run-to-run bit identity, every output element written, and the whole step —
targets, losses, backward — captured in one graph.  And the loss's positive-row scan on masks the targets kernel never writes
(pvrcnn_train_ref.SCATTER_CASES: positives scattered over lanes, waves and chunks), mask values other than 0 / 1, more and fewer
mask positives than target rows, the C entry's RoI layouts, and the targets kernel with MAX_SAMPLES samples.

Figures of the scattered cases: DESIGN.md §3.10's second table."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_train_ref as ref
from mmdet3d_gaussian_amd import _host, _lib
from test_cpu_pvrcnn_train import (MISMATCHES, check_against_restatement, check_loss_entry, check_mask_values, check_mismatch, check_scattered,
                                    check_targets_at_max_samples, check_targets_longer_than_rois, run_package)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('clockwise', [False, True])
@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_device_matches_the_restatement_and_the_twin(name, clockwise):
    inputs = ref.reference(name, clockwise)[0]
    got = run_package(inputs, clockwise, dev=DEV, form='lists')
    check_against_restatement(got, name, clockwise, 'gfx950')
    twin = run_package(inputs, clockwise, dev='cpu', form='lists')
    for k in ('label', 'reg_mask', 'label_weights', 'bbox_weights', 'pos_gt_bboxes'):   # decisions and the normalisers: the same bits
        assert torch.equal(got[k], twin[k]), k
    stacked = run_package(inputs, clockwise, dev=DEV, form='stacked')
    for k in got:                                    # one computation for both input forms, and the same bits on every run
        assert torch.equal(got[k], stacked[k]), k
    unit = run_package(inputs, clockwise, dev=DEV, form='lists', unit=True)
    assert torch.equal(unit['grad_cls'], got['grad_cls']) and all(torch.equal(unit[k], got[k]) for k in ref.LOSS_KEYS)
    assert torch.allclose(unit['grad_bbox'], got['grad_bbox'], rtol=1e-6, atol=0)       # g_l1 + g_corner: added in the kernel or by torch


def _p(t):
    return t.data_ptr() if t.numel() else None


@pytest.mark.parametrize('name', ['r1_all_positive', 'r65', 'no_positive', 'r2049'])
def test_every_output_element_is_written(name):
    """the C entry points on sentinel-filled outputs with a guard row either side: every row is written — the gradients of the rows
    that are not positive, and the targets of a batch without positives, as zeros — and nothing beyond the arrays"""
    pos, gts, ious, rois, cls_score, bbox_pred = [[t.to(DEV) for t in x] if isinstance(x, list) else x.to(DEV) for x in ref.reference(name, False)[0]]
    want = run_package(ref.reference(name, False)[0], False, dev=DEV)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    pb, pg, iu = torch.cat(pos).contiguous(), torch.cat(gts).contiguous(), torch.cat(ious).contiguous()
    pc = torch.tensor([p.shape[0] for p in pos], dtype=torch.int32, device=DEV)
    rc = torch.tensor([i.shape[0] for i in ious], dtype=torch.int32, device=DEV)
    P, R = pb.shape[0], iu.shape[0]
    S = -77.0
    label, lw, bw = (torch.full((R + 2,), S, device=DEV) for _ in range(3))
    mask = torch.full((R + 2,), -77, dtype=torch.int64, device=DEV)
    tgt = torch.full((P + 2, 7), S, device=DEV)
    _lib.check(lib.gd3d_roi_head_targets(_p(pb), _p(pg), _p(iu), _p(pc), _p(rc), pc.numel(), P, R, ref.CFG['cls_pos_thr'], ref.CFG['cls_neg_thr'], 0,
                                         label[1:].data_ptr(), tgt[1:].data_ptr(), mask[1:].data_ptr(), lw[1:].data_ptr(), bw[1:].data_ptr(), stream),
               'gd3d_roi_head_targets')
    for buf, key in ((label, 'label'), (lw, 'label_weights'), (bw, 'bbox_weights'), (mask, 'reg_mask'), (tgt, 'bbox_targets')):
        assert (buf[0] == -77).all() and (buf[-1] == -77).all(), key
        assert torch.equal(buf[1:-1].cpu(), want[key]), key
    losses = torch.full((5,), S, device=DEV)
    gc = torch.full((R + 2,), S, device=DEV)
    gb, g1, g2 = (torch.full((R + 2, 7), S, device=DEV) for _ in range(3))
    x, p, r8 = cls_score.reshape(-1).contiguous(), bbox_pred.contiguous(), rois.contiguous()
    _lib.check(lib.gd3d_roi_head_loss(_p(x), _p(p), _p(r8), 8, 1, label[1:].data_ptr(), tgt[1:].data_ptr(), _p(pg), mask[1:].data_ptr(),
                                      lw[1:].data_ptr(), bw[1:].data_ptr(), R, P, ref.LOSS_BBOX['beta'], 1.0, 1.0, 1, 0, losses[1:].data_ptr(),
                                      gc[1:].data_ptr(), gb[1:].data_ptr(), g1[1:].data_ptr(), g2[1:].data_ptr(), stream), 'gd3d_roi_head_loss')
    for buf in (losses, gc, gb, g1, g2):
        assert (buf[0] == S).all() and (buf[-1] == S).all()
        assert not (buf[1:-1] == S).any()
    assert [float(v) for v in losses[1:-1].cpu()] == [float(want[k]) for k in ref.LOSS_KEYS]
    assert torch.equal(gc[1:-1].cpu(), want['grad_cls'].reshape(-1))
    assert torch.equal(gb[1:-1].cpu(), (g1[1:-1] + g2[1:-1]).cpu())
    positive = want['reg_mask'] > 0
    assert not g1[1:-1].cpu()[~positive].any() and not g2[1:-1].cpu()[~positive].any()


@pytest.mark.parametrize('name', list(ref.SCATTER_CASES))
def test_loss_on_scattered_positives(name):
    """loss_kernel's positive-row scan — ballot and popcount inside the wave, the waves' totals through LDS, a running offset across the
    chunks of 1024 rows — on positives interleaved inside a wave, confined to some waves, absent from the first chunk, or in the last
    rows only: the restatement's result on the same permuted operands, the rows the twin pairs, the same bits on a second run"""
    got, _ = check_scattered(name, DEV)
    twin, _ = check_scattered(name, 'cpu')
    assert torch.equal(got['grad_bbox'].ne(0), twin['grad_bbox'].ne(0)) and torch.equal(got['grad_cls'].ne(0), twin['grad_cls'].ne(0))


@pytest.mark.parametrize('name', ['r2049_random', 'r65_random'])
def test_loss_takes_any_mask_value_above_zero(name):
    got, twin = check_mask_values(name, DEV), check_mask_values(name, 'cpu')
    assert torch.equal(got['grad_bbox'].ne(0), twin['grad_bbox'].ne(0))


@pytest.mark.parametrize('name', list(ref.MISMATCH_BASES))
@pytest.mark.parametrize('kind', MISMATCHES)
def test_loss_on_count_mismatches(kind, name):
    check_mismatch(kind, name, DEV)


@pytest.mark.parametrize('name', ['r2049_random', 'r65_odd_lanes'])
def test_loss_entry_writes_every_element_and_takes_any_roi_layout(name):
    """test_every_output_element_is_written's sentinels and guard rows on a scattered mask, and roi_stride / first_col of 7 / 0 and
    10 / 2 against the wrapper's 8 / 1"""
    check_loss_entry(name, DEV)


def test_targets_at_max_samples():
    """targets_kernel with both LDS tables full (B = MAX_SAMPLES = 1024): the twin's bits"""
    got, twin = check_targets_at_max_samples(DEV), check_targets_at_max_samples('cpu')
    for k in ('label', 'reg_mask', 'label_weights', 'bbox_weights', 'pos_gt_bboxes'):   # decisions and the normalisers: the same bits
        assert torch.equal(got[k], twin[k]), k


def test_targets_with_more_target_rows_than_rois():
    check_targets_longer_than_rois(DEV)


def test_whole_step_under_graph_capture():
    """targets + losses + backward with device counts and padded fixed shapes, captured in one graph (a linear sequence of launches),
    replayed once on new values in the static buffers, and compared with the eager result bit for bit"""
    name = 'b3_128_0_37'
    pos, gts, ious, rois, cls_score, bbox_pred = ref.reference(name, False)[0]
    pad_p, pad_r = 16, 27
    g = torch.Generator().manual_seed(9)
    pb = torch.cat(pos + [torch.rand(pad_p, 7, generator=g) + 0.5]).to(DEV)
    pg = torch.cat(gts + [torch.rand(pad_p, 7, generator=g) + 0.5]).to(DEV)
    iu = torch.cat(ious + [torch.rand(pad_r, generator=g)]).to(DEV)
    r8 = torch.cat([rois, torch.rand(pad_r, 8, generator=g) + 0.5]).to(DEV)
    x = torch.cat([cls_score, torch.randn(pad_r, 1, generator=g)]).to(DEV).requires_grad_(True)
    p = torch.cat([bbox_pred, torch.randn(pad_r, 7, generator=g)]).to(DEV).requires_grad_(True)
    pc = torch.tensor([q.shape[0] for q in pos], dtype=torch.int32, device=DEV)
    rc = torch.tensor([i.shape[0] for i in ious], dtype=torch.int32, device=DEV)
    unit = _host.unit_grad(torch.device(DEV))

    def step():
        tg = amd.pvrcnn_head_get_targets(pb, pg, iu, ref.CFG, pos_batch_cnt=pc, roi_batch_cnt=rc)
        losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, r8, *tg)
        vals = [losses[k] for k in ref.LOSS_KEYS]
        gx, gp = torch.autograd.grad(vals, [x, p], grad_outputs=[unit] * 3)
        return list(tg) + vals + [gx, gp]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.detach().clone() for t in step()]      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():                                 # new values in the static buffers, the counts included
        p.mul_(0.9)
        iu.mul_(0.8)
        pg[:, :3].add_(0.05)
        pc.copy_(torch.tensor([60, 0, 5], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[3], first[3]) and not torch.equal(eager[7], first[7]) and not torch.equal(eager[10], first[10])
    assert int(eager[3].sum()) == 65
    for got, want in zip(captured, eager):
        assert torch.equal(got.detach(), want.detach())
