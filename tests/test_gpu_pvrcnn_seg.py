"""PV-RCNN's keypoint segmentation slice on the MI355X (csrc/seg_head.hip): the cases of tests/test_cpu_pvrcnn_seg.py on cuda:0.  n_pos and
the winner columns bit-identical to the `_cpu` twin and to the fp32 restatement, the loss, the gradients and the reweighted features
within the same bounds against the fp64 restatement (computed on the CPU, once per case), run-to-run bit identity, the 16-byte and the
4-byte access paths bit-identical, every output element written, and the keypoint step — mask targets, seg loss, reweighting, backward
— captured in one graph.

Figures: every case passes on gfx950; the largest |ours - fp64| / bound per tensor is in DESIGN.md §3.12's table."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_seg_ref as ref
from mmdet3d_gaussian_amd import _lib
from test_cpu_pvrcnn_seg import (SINGLE_SHIFTS, check_entries_equal_the_wrapper, check_foreign_winner_bytes, check_loss_case,
                                  check_one_sided_backward, check_reweight_case, check_single_misaligned_operand, run_loss, run_reweight)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', sorted(ref.LOSS_CASES))
def test_seg_loss_on_the_device(name):
    case = ref.loss_reference(name)[0]
    got = run_loss(case, dev=DEV)
    check_loss_case(got, name, 'gfx950')
    twin = run_loss(case, dev='cpu')
    assert torch.equal(got['n_pos'], twin['n_pos'])                       # the count: the same bits
    again = run_loss(case, dev=DEV, unit=True)                            # the same bits on every run, and through the unit-gradient path
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('name', ref.ALL_REWEIGHT_CASES)
def test_reweight_on_the_device(name):
    """with the two sweep cases (pvrcnn_seg_ref.EXTRA_REWEIGHT_CASES: N = 32773 > 8192 workgroups x 4 rows) the second trip of the
    grid-stride loop of reweight_kernel<true>, reweight_kernel<false> and both reweight_backward_kernel instances runs here"""
    case = ref.reweight_reference(name)[0]
    got = run_reweight(case, dev=DEV)
    check_reweight_case(got, name, 'gfx950')
    twin = run_reweight(case, dev='cpu')
    assert torch.equal(got['win'], twin['win'])
    again = run_reweight(case, dev=DEV)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_reweight_misaligned_base_equals_the_aligned_case():
    """C = 128 with every (N, C) operand viewed one float into a larger buffer: the 4-byte path gives the 16-byte path's bits"""
    case = ref.reweight_reference(ref.MISALIGNED_OF)[0]
    aligned, shifted = run_reweight(case, dev=DEV), run_reweight(case, dev=DEV, view=ref.offset_view)
    for k in aligned:
        assert torch.equal(aligned[k], shifted[k]), k


@pytest.mark.parametrize('name', ['n65_k1', 'n65_k3', 'n2049_k1', 'n2049_k3', 'all_ignored_k1', 'all_ignored_k3'])
def test_every_loss_output_element_is_written(name):
    """the C entry point on sentinel-filled outputs with a guard row either side: every gradient row is written — zeros on the rows of
    weight 0 — and nothing beyond the arrays"""
    case = ref.loss_reference(name)[0]
    want = run_loss(case, dev=DEV)
    x, t = case['seg_preds'].to(DEV).contiguous(), case['seg_targets'].to(DEV).contiguous()
    N, K = x.shape
    S = -77.0
    out = torch.full((4,), S, device=DEV)
    grad = torch.full((N + 2, K), S, device=DEV)
    cfg = case['cfg']
    _lib.check(_lib.load().gd3d_seg_head_loss(x.data_ptr(), t.data_ptr(), N, K, ref.NUM_CLASSES, int(case['class_agnostic']), cfg['gamma'], cfg['alpha'],
                                              cfg['loss_weight'], out[1:].data_ptr(), grad[1:].data_ptr(), torch.cuda.current_stream().cuda_stream),
               'gd3d_seg_head_loss')
    for buf in (out, grad):
        assert (buf[0] == S).all() and (buf[-1] == S).all()
        assert not (buf[1:-1] == S).any()
    assert float(out[1]) == float(want['loss']) and float(out[2]) == float(want['n_pos'])
    assert torch.equal(grad[1:-1].cpu(), want['grad'])
    if name.startswith('all_ignored'):
        assert not grad[1:-1].any() and float(out[1]) == 0.0


@pytest.mark.parametrize('name', ['n65_c3_k3', 'n67_c260_k3'])
def test_every_reweight_output_element_is_written(name):
    case = ref.reweight_reference(name)[0]
    want = run_reweight(case, dev=DEV)
    f, x, g = (case[k].to(DEV).contiguous() for k in ('feats', 'seg_preds', 'grad_out'))
    N, C = f.shape
    K = x.size(1)
    S = -77.0
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    out, gf = torch.full((N + 2, C), S, device=DEV), torch.full((N + 2, C), S, device=DEV)
    gx = torch.full((N + 2, K), S, device=DEV)
    win = torch.full((N + 2,), 200, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gd3d_keypoint_reweight(f.data_ptr(), x.data_ptr(), N, C, K, out[1:].data_ptr(), win[1:].data_ptr(), stream), 'gd3d_keypoint_reweight')
    _lib.check(lib.gd3d_keypoint_reweight_backward(g.data_ptr(), f.data_ptr(), x.data_ptr(), win[1:].data_ptr(), N, C, K, gf[1:].data_ptr(),
                                                   gx[1:].data_ptr(), stream), 'gd3d_keypoint_reweight_backward')
    for buf in (out, gf, gx):
        assert (buf[0] == S).all() and (buf[-1] == S).all()
        assert not (buf[1:-1] == S).any()
    assert win[0] == 200 and win[-1] == 200 and (win[1:-1] < K).all()
    assert torch.equal(out[1:-1].cpu(), want['out']) and torch.equal(win[1:-1].cpu().long(), want['win'])
    assert torch.equal(gf[1:-1].cpu(), want['grad_feats']) and torch.equal(gx[1:-1].cpu(), want['grad_seg'])


@pytest.mark.parametrize('name', ['n130_c8_k255'] + list(ref.SWEEP_CASES))
def test_reweight_entry_points_write_every_element_and_nothing_beyond(name):
    """as test_every_reweight_output_element_is_written, on K = 255 and on the two sweep cases: the rows of the second trip (N = 32773 =
    8192 workgroups x 4 rows + 5) are written like every other row, and the guard row past them is not"""
    check_entries_equal_the_wrapper(name, DEV)


@pytest.mark.parametrize('shift', SINGLE_SHIFTS)
def test_reweight_single_misaligned_operand_equals_the_aligned_run(shift):
    check_single_misaligned_operand(shift, DEV)


@pytest.mark.parametrize('name', ['n65_c3_k3', 'n130_c128_k3'])
def test_reweight_backward_clamps_a_foreign_winner_byte(name):
    """run on the `_cpu` twin first (tests/test_cpu_pvrcnn_seg.py): the clamp is documented behaviour, checked with guard rows"""
    check_foreign_winner_bytes(name, DEV)


def test_reweight_one_sided_backward_equals_the_two_sided_run():
    check_one_sided_backward('n130_c128_k3', DEV)


def test_keypoint_step_under_graph_capture():
    """pointwise_mask_targets -> pvrcnn_seg_loss -> keypoint_reweight -> the gradients of the loss plus a fixed linear functional of the
    reweighted features, for 2 samples x 96 keypoints, 5 gt boxes each, C = 8: captured in one graph (a linear sequence of launches),
    replayed once on new values in the static buffers (logits, boxes, keypoints), and compared with the eager step bit for bit"""
    B, P, T, C, K = 2, 96, 5, 8, ref.NUM_CLASSES
    g = torch.Generator().manual_seed(11)
    boxes = torch.cat([torch.rand(B, T, 2, generator=g) * 16 - 8, torch.rand(B, T, 1, generator=g) - 1.5,
                       torch.rand(B, T, 3, generator=g) * torch.tensor([2.0, 1.0, 0.5]) + torch.tensor([3.0, 1.4, 1.4]),
                       (torch.rand(B, T, 1, generator=g) * 2 - 1) * 3.14], dim=-1)
    labels = torch.randint(0, ref.NUM_CLASSES, (B, T), generator=g)
    owner = torch.randint(0, T, (B, P), generator=g)
    near = torch.gather(boxes[..., :3], 1, owner[..., None].expand(-1, -1, 3)) + torch.randn(B, P, 3, generator=g) * torch.tensor([1.2, 0.6, 0.5]) \
        + torch.tensor([0.0, 0.0, 0.7])
    far = torch.rand(B, P, 3, generator=g) * torch.tensor([30.0, 30.0, 3.0]) - torch.tensor([15.0, 15.0, 2.0])
    xyz = torch.where(torch.rand(B, P, 1, generator=g) < 0.6, near, far).reshape(B * P, 3).to(DEV)
    boxes, labels = boxes.to(DEV), labels.to(DEV)
    cnt = torch.full((B,), P, dtype=torch.int32, device=DEV)
    box_cnt = torch.full((B,), T, dtype=torch.int32, device=DEV)
    x = ref.gapped_logits(B * P, K, g).to(DEV).requires_grad_(True)
    feats = torch.randn(B * P, C, generator=g).to(DEV).requires_grad_(True)
    functional = torch.randn(B * P, C, generator=g).to(DEV)

    def step():
        seg = amd.pointwise_mask_targets(xyz, cnt, boxes, labels, 0.2, ref.NUM_CLASSES, box_cnt=box_cnt)
        loss = amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, seg, ref.NUM_CLASSES)['loss_seg']
        out = amd.keypoint_reweight(feats, x)
        gf, gx = torch.autograd.grad(loss + (out * functional).sum(), [feats, x])
        return [seg, loss, out, gf, gx]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.detach().clone() for t in step()]      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    seg0 = first[0].cpu()
    assert ((seg0 >= 0) & (seg0 < ref.NUM_CLASSES)).any() and (seg0 == -1).any() and (seg0 == ref.NUM_CLASSES).any()   # every kind of row
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():                                 # new values in the static buffers
        x.mul_(0.9)
        boxes[..., :2].add_(0.4)
        xyz[:, 2].add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[0], first[0])            # the replayed targets differ from the first step's
    assert not torch.equal(eager[1].detach(), first[1]) and not torch.equal(eager[4], first[4])
    for got, want in zip(captured, eager):
        assert torch.equal(got.detach(), want.detach())
