"""PVRCNNBboxHead's training slice through the `_cpu` twins (csrc/roi_head_cpu.cpp): `pvrcnn_head_get_targets` and `pvrcnn_head_loss`
against the statement-by-statement torch restatement of the reference (tests/pvrcnn_train_ref.py).

  * decisions — label, label_weights > 0, reg_mask — bit-exact against the fp32 restatement;
  * loss values within 1e-5 (relative) of the fp64 restatement;
  * bbox_targets, the normalised weights and both gradients within 4x the fp32 restatement's own largest deviation from the fp64 one
    on the same inputs (printed per case; DESIGN.md §3.10 records the figures);
on the smallest shapes that cross a boundary (pvrcnn_train_ref.CASES), both rotation senses, both input forms; and the loss alone on
scattered positives (pvrcnn_train_ref.SCATTER_CASES), other mask values, count mismatches and the C entry's RoI layouts — the checks
tests/test_gpu_pvrcnn_train.py repeats on the device, with every generator condition asserted here."""
import math

import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_train_ref as ref
from mmdet3d_gaussian_amd import _host


def run_package(inputs, clockwise, dev='cpu', form='lists', with_corner_loss=True, unit=False, dtype=torch.float32):
    """targets + losses + the gradients of the summed losses through the package on `dev` -> dict like pvrcnn_train_ref.evaluate's"""
    pos, gts, ious, rois, cls_score, bbox_pred = [[t.to(dev, dtype) for t in x] if isinstance(x, list) else x.to(dev, dtype) for x in inputs]
    if form == 'lists':
        tg = amd.pvrcnn_head_get_targets(pos, gts, ious, ref.CFG, clockwise=clockwise)
    else:
        pc = torch.tensor([p.shape[0] for p in pos], dtype=torch.int64).to(dev)
        rc = torch.tensor([i.shape[0] for i in ious], dtype=torch.int32).to(dev)
        tg = amd.pvrcnn_head_get_targets(torch.cat(pos), torch.cat(gts), torch.cat(ious), ref.CFG, pos_batch_cnt=pc, roi_batch_cnt=rc,
                                         clockwise=clockwise)
    x = cls_score.clone().requires_grad_(True)
    p = bbox_pred.clone().requires_grad_(True)
    losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, rois, *tg, with_corner_loss=with_corner_loss, clockwise=clockwise)
    if unit:
        vals = list(losses.values())
        torch.autograd.backward(vals, grad_tensors=[_host.unit_grad(vals[0].device)] * len(vals))
    else:
        sum(losses.values()).backward()
    out = dict(zip(('label', 'bbox_targets', 'pos_gt_bboxes', 'reg_mask', 'label_weights', 'bbox_weights'), tg))
    out.update({k: v.detach() for k, v in losses.items()})
    out['grad_cls'], out['grad_bbox'] = x.grad, p.grad
    return {k: v.cpu() for k, v in out.items()}


def check_against_restatement(got, name, clockwise, what):
    """the assertions the CPU and the GPU file share; prints every measured figure before it asserts"""
    _, r32, r64 = ref.reference(name, clockwise)
    assert got['label'].dtype == torch.float32 and got['reg_mask'].dtype == torch.int64
    assert torch.equal(got['label'], r32['label']), f'{what}: label differs from the fp32 restatement'
    assert torch.equal(got['reg_mask'], r32['reg_mask'])
    assert torch.equal(got['label_weights'] > 0, r32['label_weights'] > 0)
    assert torch.equal(got['pos_gt_bboxes'], r32['pos_gt_bboxes'])
    failures = []
    for k, (dev32, bound) in ref.bounds(name, clockwise).items():
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        err = float((got[k].double() - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f'{what} {name} clockwise={clockwise} {k}: |ours - fp64| = {err:.3e}; fp32 restatement {dev32:.3e}; bound {bound:.3e}')
        if not err <= bound:
            failures.append((k, err, bound))
    for k in ref.LOSS_KEYS:
        want = float(r64[k])
        err = abs(float(got[k]) - want)
        print(f'{what} {name} clockwise={clockwise} {k}: ours {float(got[k]):.9g}, fp64 {want:.9g}, relative error '
              f'{err / abs(want) if want else err:.3e} (bar {ref.LOSS_RTOL:g})')
        if not err <= ref.LOSS_RTOL * abs(want):
            failures.append((k, err, ref.LOSS_RTOL * abs(want)))
    assert not failures, f'{what} {name} clockwise={clockwise}: (key, error, bound) {failures}'


@pytest.mark.parametrize('clockwise', [False, True])
@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_generator_keeps_its_margins(name, clockwise):
    """the committed seeds keep every corner away from the tie of the two distances and from a zero distance (fp64 restatement), and
    the yaw difference away from the quadrant borders in all four quadrants"""
    tie, zero = ref.tie_margins(name, clockwise)
    assert tie > ref.TIE_MARGIN and zero > ref.TIE_MARGIN, (tie, zero)
    pos, gts = ref.reference(name, clockwise)[0][:2]
    u = torch.remainder(torch.cat(gts)[:, 6].double() - torch.cat(pos)[:, 6].double(), 2 * math.pi)
    for border in (math.pi / 2, math.pi, 3 * math.pi / 2):
        assert u.numel() == 0 or float((u - border).abs().min()) >= 1e-3
    if u.numel() >= 64:
        assert sorted(set((u / (math.pi / 2)).floor().long().tolist())) == [0, 1, 2, 3]


@pytest.mark.parametrize('clockwise', [False, True])
@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_cpu_twin_matches_the_restatement(name, clockwise):
    inputs = ref.reference(name, clockwise)[0]
    lists = run_package(inputs, clockwise, form='lists')
    check_against_restatement(lists, name, clockwise, 'cpu twin')
    stacked = run_package(inputs, clockwise, form='stacked')
    for k in lists:                                  # the two input forms are one computation
        assert torch.equal(lists[k], stacked[k]), k
    again = run_package(inputs, clockwise, form='lists')
    for k in lists:                                  # and the same bits on every run
        assert torch.equal(lists[k], again[k]), k


# ---- scattered positives, mask values, count mismatches, the C entry's RoI layout, B = MAX_SAMPLES ------------------------------------

SENTINEL = -77.0
MISMATCHES = ('more_positives', 'fewer_positives', 'longer_target_buffer')


def run_loss(case, dev='cpu'):
    """`pvrcnn_head_loss` and the gradients of the summed losses on loss operands (pvrcnn_train_ref.scatter's dict) -> dict on the CPU"""
    t = {k: case[k].to(dev) for k in ref.LOSS_INPUT_KEYS}
    x, p = t['cls_score'].clone().requires_grad_(True), t['bbox_pred'].clone().requires_grad_(True)
    losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, t['rois'], t['label'], t['bbox_targets'], t['pos_gt_bboxes'], t['reg_mask'],
                                  t['label_weights'], t['bbox_weights'])
    sum(losses.values()).backward()
    out = {k: v.detach().cpu() for k, v in losses.items()}
    out['grad_cls'], out['grad_bbox'] = x.grad.cpu(), p.grad.cpu()
    return out


def check_loss_against(got, r32, r64, what):
    """the project's rule on a loss-only evaluation: loss values within LOSS_RTOL of fp64, gradients within NOISE_FACTOR times the fp32
    restatement's own deviation; prints every figure before it asserts -> {key: (error, fp32 restatement's deviation, bound)}"""
    failures, figures = [], {}
    for k, (dev32, bound) in ref.loss_bounds(r32, r64).items():
        assert got[k].shape == r64[k].shape and got[k].dtype == torch.float32, (k, got[k].shape, r64[k].shape)
        err = float((got[k].double() - r64[k]).abs().max())
        print(f'{what} {k}: |ours - fp64| = {err:.3e}; fp32 restatement {dev32:.3e}; bound {bound:.3e}; ratio to bound {err / bound if bound else 0.0:.3f}')
        figures[k] = (err, dev32, bound)
        if not err <= bound:
            failures.append((k, err, bound))
    for k in ref.LOSS_KEYS:
        want = float(r64[k])
        err = abs(float(got[k]) - want)
        print(f'{what} {k}: ours {float(got[k]):.9g}, fp64 {want:.9g}, relative error {err / abs(want) if want else err:.3e} (bar {ref.LOSS_RTOL:g})')
        figures[k] = (err / abs(want) if want else err, 0.0, ref.LOSS_RTOL)
        if not err <= ref.LOSS_RTOL * abs(want):
            failures.append((k, err, ref.LOSS_RTOL * abs(want)))
    assert not failures, f'{what}: (key, error, bound) {failures}'
    return figures


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), k


def check_scattered(name, dev='cpu'):
    """a scattered case on `dev`: within the bounds of the restatement on the same permuted operands, a bbox_pred gradient on exactly the
    positive rows, and the same bits on a second run -> (the result, the figures)"""
    case, r32, r64 = ref.scattered_reference(name)
    got = run_loss(case, dev)
    figures = check_loss_against(got, r32, r64, f'{dev} {name}')
    assert torch.equal(got['grad_bbox'].ne(0).any(dim=1), case['reg_mask'] > 0), 'the rows that pair with a target are the positive rows'
    assert torch.equal(r64['grad_bbox'].ne(0).any(dim=1), case['reg_mask'] > 0)
    same_bits(got, run_loss(case, dev))
    return got, figures


def check_mask_values(name, dev='cpu'):
    """positives carry 1, 2, 7, every third other row -1: the rule is reg_mask > 0, so the result has the 0 / 1 mask's bits"""
    case, r32, r64 = ref.scattered_reference(name)
    valued = ref.with_mask_values(case)
    v64 = ref.evaluate_loss(valued, torch.float64)
    same_bits(v64, r64)                                       # the expectation is unchanged
    got = run_loss(valued, dev)
    check_loss_against(got, r32, r64, f'{dev} {name} mask values 1, 2, 7, -1')
    same_bits(got, run_loss(case, dev))
    return got


def check_mismatch(kind, name, dev='cpu'):
    """the documented behaviour of `pvrcnn_head_loss` when mask positives and target rows do not match in number"""
    case, r32, r64 = ref.scattered_reference(name)
    matched = run_loss(case, dev)
    P, R = case['bbox_targets'].size(0), case['reg_mask'].numel()
    n = 10 if R > 1000 else 5
    if kind == 'more_positives':            # positives past the P-th are ignored
        more, extra = ref.with_extra_positives(case, n)
        got = run_loss(more, dev)
        same_bits(got, matched, ref.LOSS_KEYS)              # the three losses: the matched call's bits (the corner mean runs over P rows)
        assert not got['grad_bbox'][extra].any() and not matched['grad_bbox'][extra].any()
        same_bits(got, matched, ('grad_cls', 'grad_bbox'))  # every gradient row, the extra ones included (zeros in both)
        check_loss_against(got, r32, r64, f'{dev} {name} {n} extra positives')
    elif kind == 'fewer_positives':         # the paired rows are the positives there are: the corner mean runs over P - n rows
        ours, theirs, cleared = ref.with_fewer_positives(case, n)
        got = run_loss(ours, dev)
        t32, t64 = ref.evaluate_loss(theirs, torch.float32), ref.evaluate_loss(theirs, torch.float64)
        check_loss_against(got, t32, t64, f'{dev} {name} {n} positives cleared')
        assert not got['grad_bbox'][cleared].any() and matched['grad_bbox'][cleared].ne(0).any(dim=1).all()
        same_bits(got, run_loss(theirs, dev))               # and the same bits as the call with the buffers cut to P - n rows
        assert not torch.equal(got['loss_corner'], matched['loss_corner'])
    elif kind == 'longer_target_buffer':    # P > R: rows of the buffers no positive reaches
        longer = ref.with_longer_target_buffer(case, R)
        assert longer['bbox_targets'].size(0) == P + R > R
        same_bits(run_loss(longer, dev), matched)
    else:
        raise KeyError(kind)


def loss_entry(case, dev='cpu', stride=8, first=1):
    """`gd3d_roi_head_loss` (or its twin) on sentinel-filled outputs with a guard row either side, the RoI boxes at column `first` of rows
    of `stride` floats (the other columns hold a value no box has).  Asserts every element written and no guard -> dict on the CPU"""
    t = {k: case[k].to(dev).contiguous() for k in ref.LOSS_INPUT_KEYS}
    R, P = t['reg_mask'].numel(), t['bbox_targets'].size(0)
    rois = torch.full((R, stride), 1e6, device=dev)
    rois[:, first:first + 7] = t['rois'][:, 1:8]
    losses = torch.full((5,), SENTINEL, device=dev)
    gc = torch.full((R + 2,), SENTINEL, device=dev)
    gb, g1, g2 = (torch.full((R + 2, 7), SENTINEL, device=dev) for _ in range(3))
    _host.call('gd3d_roi_head_loss', rois.device,
               (t['cls_score'].data_ptr(), t['bbox_pred'].data_ptr(), rois.data_ptr(), stride, first, t['label'].data_ptr(), t['bbox_targets'].data_ptr(),
                t['pos_gt_bboxes'].data_ptr(), t['reg_mask'].data_ptr(), t['label_weights'].data_ptr(), t['bbox_weights'].data_ptr(), R, P,
                ref.LOSS_BBOX['beta'], 1.0, 1.0, 1, 0, losses[1:].data_ptr(), gc[1:].data_ptr(), gb[1:].data_ptr(), g1[1:].data_ptr(), g2[1:].data_ptr()))
    for buf in (losses, gc, gb, g1, g2):
        assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), 'a guard was written'
        assert not (buf[1:-1] == SENTINEL).any(), 'an output element was left unwritten'
    out = dict(zip(ref.LOSS_KEYS, losses[1:-1].cpu()))
    out.update(grad_cls=gc[1:-1].cpu().reshape(-1, 1), grad_bbox=gb[1:-1].cpu(), grad_l1=g1[1:-1].cpu(), grad_corner=g2[1:-1].cpu())
    return out


def check_loss_entry(name, dev='cpu'):
    """a scattered case through the C entry: every output element written and nothing beyond, the wrapper's bits, and the RoI layouts
    7 / 0 and 10 / 2 giving the bits of the reference's 8 / 1"""
    case = ref.scattered_reference(name)[0]
    want = run_loss(case, dev)
    base = loss_entry(case, dev, 8, 1)
    same_bits(base, want, ref.LOSS_KEYS + ('grad_cls',))
    assert torch.equal(base['grad_bbox'], base['grad_l1'] + base['grad_corner'])
    other = case['reg_mask'] <= 0
    assert not base['grad_l1'][other].any() and not base['grad_corner'][other].any() and base['grad_corner'][~other].ne(0).any(dim=1).all()
    for stride, first in ((7, 0), (10, 2)):
        same_bits(loss_entry(case, dev, stride, first), base)


def check_targets_at_max_samples(dev='cpu'):
    """B = MAX_SAMPLES = 1024 samples over the 2049 rows of case r2049: its three samples at indices 3, 511 and 1023, every other one
    with roi_cnt = pos_cnt = 0.  Equal to the list form over the non-empty samples — the restatement's decisions, its values within the
    case's bounds, and the list form's bits"""
    name = 'r2049'
    pos, gts, ious = ref.reference(name, False)[0][:3]
    _, r32, r64 = ref.reference(name, False)
    pc, rc = torch.zeros(1024, dtype=torch.int32), torch.zeros(1024, dtype=torch.int32)
    for at, p, i in zip((3, 511, 1023), pos, ious):
        pc[at], rc[at] = p.size(0), i.size(0)
    assert int((rc > 0).sum()) == 3 and int(rc.sum()) == 2049 and int((pc > 0).sum()) == 3
    keys = ('label', 'bbox_targets', 'pos_gt_bboxes', 'reg_mask', 'label_weights', 'bbox_weights')
    got = dict(zip(keys, (t.cpu() for t in amd.pvrcnn_head_get_targets(torch.cat(pos).to(dev), torch.cat(gts).to(dev), torch.cat(ious).to(dev), ref.CFG,
                                                                       pos_batch_cnt=pc.to(dev), roi_batch_cnt=rc.to(dev)))))
    lists = dict(zip(keys, (t.cpu() for t in amd.pvrcnn_head_get_targets([p.to(dev) for p in pos], [g.to(dev) for g in gts], [i.to(dev) for i in ious], ref.CFG))))
    same_bits(got, lists)
    for k in ('label', 'reg_mask', 'pos_gt_bboxes'):
        assert torch.equal(got[k], r32[k]), k
    assert torch.equal(got['label_weights'] > 0, r32['label_weights'] > 0)
    for k in ('bbox_targets', 'label_weights', 'bbox_weights'):
        dev32, bound = ref.bounds(name, False)[k]
        err = float((got[k].double() - r64[k]).abs().max())
        print(f'{dev} {name} over 1024 samples {k}: |ours - fp64| = {err:.3e}; fp32 restatement {dev32:.3e}; bound {bound:.3e}')
        assert err <= bound, (k, err, bound)
    return got


@pytest.mark.parametrize('name', list(ref.SCATTER_CASES) + list(ref.MISMATCH_BASES))
def test_scattered_generator_keeps_its_margins(name):
    """a permutation of rows leaves the generator's margins where test_generator_keeps_its_margins finds them; asserted on the permuted
    operands all the same, and the pattern's own condition with them"""
    case = ref.scattered_reference(name)[0]
    tie, zero = ref.scattered_margins(case)
    assert tie > ref.TIE_MARGIN and zero > ref.TIE_MARGIN, (tie, zero)
    pos, gts = case['drawn']
    u = torch.remainder(torch.cat(gts)[:, 6].double() - torch.cat(pos)[:, 6].double(), 2 * math.pi)
    for border in (math.pi / 2, math.pi, 3 * math.pi / 2):
        assert float((u - border).abs().min()) >= 1e-3
    if u.numel() >= 64:
        assert sorted(set((u / (math.pi / 2)).floor().long().tolist())) == [0, 1, 2, 3]
    R, pattern = ref.SCATTER_ALL[name]
    rows = torch.arange(R)[case['reg_mask'] > 0]
    P = rows.numel()
    assert R == case['reg_mask'].numel() and P == case['bbox_targets'].size(0) >= 1
    if pattern == 'random':
        assert (rows % 2 == 0).any() and (rows % 2 == 1).any() and (P >= 19) and not torch.equal(rows, torch.arange(P))
    if pattern == 'odd_lanes':
        assert (rows % 64 % 2 == 1).all() and P >= 19
    if pattern == 'odd_waves':
        assert (rows // 64 % 2 == 1).all() and (P == 1 or (rows < 1024).any() and (rows >= 1024).any())
    if pattern == 'from_1024':
        assert (rows >= 1024).all() and P > 1
    if pattern == 'last64_and_2048':
        assert rows.tolist() == list(range(1984, 2049))
    if pattern == 'all_positive':
        assert P == R
    if pattern == 'random_head':
        assert R - 1 - int(rows.max()) >= 10


@pytest.mark.parametrize('name', list(ref.SCATTER_CASES))
def test_loss_twin_on_scattered_positives(name):
    check_scattered(name)


@pytest.mark.parametrize('name', ['r2049_random', 'r65_random'])
def test_loss_twin_takes_any_mask_value_above_zero(name):
    check_mask_values(name)


@pytest.mark.parametrize('name', list(ref.MISMATCH_BASES))
@pytest.mark.parametrize('kind', MISMATCHES)
def test_loss_twin_on_count_mismatches(kind, name):
    check_mismatch(kind, name)


@pytest.mark.parametrize('name', ['r2049_random', 'r65_odd_lanes'])
def test_loss_twin_entry_writes_every_element_and_takes_any_roi_layout(name):
    check_loss_entry(name)


def test_targets_twin_at_max_samples():
    check_targets_at_max_samples()


def test_targets_twin_with_more_target_rows_than_rois():
    check_targets_longer_than_rois()


def check_targets_longer_than_rois(dev='cpu'):
    """stacked inputs whose positive buffers are padded past the RoI rows (P = 73 > R = 64: the launch is sized by the larger): the
    covered rows are the exact call's, the target rows past the counts zeros"""
    pos, gts, ious = ref.reference('r64_all_positive', False)[0][:3]
    exact = amd.pvrcnn_head_get_targets([p.to(dev) for p in pos], [g.to(dev) for g in gts], [i.to(dev) for i in ious], ref.CFG)
    g = torch.Generator().manual_seed(6)
    pb = torch.cat(pos + [torch.rand(9, 7, generator=g) + 0.5]).to(dev)
    pg = torch.cat(gts + [torch.rand(9, 7, generator=g) + 0.5]).to(dev)
    cnt = torch.tensor([64], dtype=torch.int32, device=dev)
    got = amd.pvrcnn_head_get_targets(pb, pg, torch.cat(ious).to(dev), ref.CFG, pos_batch_cnt=cnt, roi_batch_cnt=cnt)
    assert got[1].shape == (73, 7) and torch.equal(got[1][:64], exact[1]) and not got[1][64:].any()
    for k in (0, 3, 4, 5):
        assert got[k].shape == (64,) and torch.equal(got[k], exact[k]), k


def _single(roi_yaw, gt_yaw, clockwise=False):
    roi = torch.tensor([[1.0, 2.0, 0.0, 2.0, 1.0, 1.5, roi_yaw]])
    off = (1.0, 0.5, 0.25)
    gt = torch.tensor([[1.0 + off[0], 2.0 + off[1], 0.0 + off[2], 2.2, 0.9, 1.2, gt_yaw]])
    t = amd.pvrcnn_head_get_targets([roi], [gt], [torch.tensor([0.9])], ref.CFG, clockwise=clockwise)[1][0].double()
    ry = math.fmod(float(roi[0, 6]), 2 * math.pi)
    ry = ry + 2 * math.pi if ry < 0 else ry
    s = -math.sin(ry) if clockwise else math.sin(ry)
    x = off[0] * math.cos(ry) + off[1] * s
    y = -off[0] * s + off[1] * math.cos(ry)
    diag = math.sqrt(1.0 ** 2 + 2.0 ** 2)
    head = [x / diag, y / diag, ((off[2] + 1.2 / 2) - 1.5 / 2) / 1.5, math.log(2.2 / 2.0), math.log(0.9 / 1.0), math.log(1.2 / 1.5)]
    assert torch.allclose(t[:6], torch.tensor(head, dtype=torch.float64), rtol=0, atol=2e-6), (t[:6], head)
    return float(t[6])


@pytest.mark.parametrize('clockwise', [False, True])
def test_hand_computed_target_branches(clockwise):
    """one RoI, one gt, by hand: the canonical offset and dims, and the yaw through each of its four branches"""
    assert abs(_single(0.3, 0.3 + 0.5, clockwise) - 0.5) < 1e-6                        # first quadrant: as it is
    assert abs(_single(0.3, 0.3 + 2.0, clockwise) - (2.0 - math.pi)) < 1e-6            # opposite: + pi, then > pi: - 2 pi
    assert abs(_single(0.3, 0.3 + 5.5, clockwise) - (5.5 - 2 * math.pi)) < 1e-6        # fourth quadrant: > pi mapped down
    assert abs(_single(-0.3 - 2 * math.pi, -0.3 + 0.5, clockwise) - 0.5) < 2e-6        # a negative roi yaw wraps up first
    # r == fp32(3 pi / 2) is not 'opposite' (strict <); r - fp32(2 pi) falls just below -fp32(pi / 2): the clamp brings it back
    three_half_pi = float(torch.tensor(1.5 * math.pi, dtype=torch.float32))
    half_pi = float(torch.tensor(0.5 * math.pi, dtype=torch.float32))
    assert three_half_pi - float(torch.tensor(2 * math.pi, dtype=torch.float32)) < -half_pi
    assert _single(0.0, three_half_pi, clockwise) == -half_pi
    # labels: above, between, below the thresholds, and the thresholds themselves (strict comparisons)
    iou = torch.tensor([0.8, 0.5, 0.1, 0.75, 0.25])
    roi = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]])
    label, _, _, mask, lw, bw = amd.pvrcnn_head_get_targets([roi], [roi], [iou], ref.CFG)
    assert label.tolist() == [1.0, 0.5, 0.0, 1.0, 0.0] and mask.tolist() == [1, 0, 0, 0, 0]
    assert torch.equal(lw, torch.ones(5) / 5) and bw.tolist() == [1.0, 0, 0, 0, 0]
    label = amd.pvrcnn_head_get_targets([roi], [roi], [torch.tensor([0.3, 0.2])], dict(cls_pos_thr=0.75, cls_neg_thr=0.1))
    assert torch.equal(label[0], torch.tensor([0.3, 0.2]) * 2 - 0.5) and label[0][1] < 0 and label[4].tolist() == [1.0, 0.0]   # a negative label is weightless


def test_padded_rows_are_weightless_and_counts_are_clamped():
    """stacked inputs whose counts do not cover the rows (fixed shapes for a captured graph): same targets on the covered rows, zeros
    past them, and the loss of the padded step equals the loss of the exact one; a count beyond the rows left is cut"""
    name = 'b3_128_0_37'
    pos, gts, ious, rois, cls_score, bbox_pred = ref.reference(name, False)[0]
    exact = run_package(ref.reference(name, False)[0], False, form='stacked')
    P, R = sum(p.shape[0] for p in pos), rois.shape[0]
    pad_p, pad_r = 9, 30
    g = torch.Generator().manual_seed(5)
    pb = torch.cat(pos + [torch.rand(pad_p, 7, generator=g) + 0.5])
    pg = torch.cat(gts + [torch.rand(pad_p, 7, generator=g) + 0.5])
    iu = torch.cat(ious + [torch.rand(pad_r, generator=g)])
    pc = torch.tensor([p.shape[0] for p in pos], dtype=torch.int32)
    rc = torch.tensor([i.shape[0] for i in ious], dtype=torch.int32)
    tg = amd.pvrcnn_head_get_targets(pb, pg, iu, ref.CFG, pos_batch_cnt=pc, roi_batch_cnt=rc)
    for got, key in zip(tg, ('label', 'bbox_targets', None, 'reg_mask', 'label_weights', 'bbox_weights')):
        if key is not None:
            n = exact[key].shape[0]
            assert torch.equal(got[:n], exact[key]) and not got[n:].any() and got.shape[0] == n + (pad_p if key == 'bbox_targets' else pad_r)
    rois_p = torch.cat([rois, torch.rand(pad_r, 8, generator=g) + 0.5])
    x = torch.cat([cls_score, torch.randn(pad_r, 1, generator=g)]).requires_grad_(True)
    p = torch.cat([bbox_pred, torch.randn(pad_r, 7, generator=g)]).requires_grad_(True)
    losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, rois_p, *tg)
    sum(losses.values()).backward()
    for k in ref.LOSS_KEYS:
        assert torch.equal(losses[k].detach(), exact[k]), k
    assert torch.equal(x.grad[:R], exact['grad_cls']) and not x.grad[R:].any()
    assert torch.equal(p.grad[:R], exact['grad_bbox']) and not p.grad[R:].any()
    over = amd.pvrcnn_head_get_targets(torch.cat(pos), torch.cat(gts), torch.cat(ious), ref.CFG,
                                       pos_batch_cnt=torch.tensor([64, 0, 1 << 30]), roi_batch_cnt=torch.tensor([128, -4, 1 << 30]))
    assert torch.equal(over[3], exact['reg_mask']) and torch.equal(over[0], exact['label'])


def test_unit_gradient_corner_switch_and_other_dtypes():
    name = 'r65'
    inputs = ref.reference(name, False)[0]
    base = run_package(inputs, False)
    unit = run_package(inputs, False, unit=True)                 # the stored gradients as they are: nothing is scaled
    assert torch.equal(unit['grad_cls'], base['grad_cls'])
    assert torch.allclose(unit['grad_bbox'], base['grad_bbox'], rtol=1e-6, atol=0)     # g_l1 + g_corner, added in the kernel or by torch
    plain = run_package(inputs, False, with_corner_loss=False)
    assert 'loss_corner' not in plain and torch.equal(plain['loss_bbox'], base['loss_bbox']) and torch.equal(plain['loss_cls'], base['loss_cls'])
    r64 = ref.evaluate(inputs, torch.float64, False, with_corner_loss=False)
    bound = ref.bounds(name, False)['grad_bbox'][1]
    assert float((plain['grad_bbox'].double() - r64['grad_bbox']).abs().max()) <= bound
    dbl = run_package(inputs, False, dtype=torch.float64)        # evaluated in fp32, cast back
    assert dbl['grad_bbox'].dtype == torch.float64 and dbl['loss_cls'].dtype == torch.float64 and dbl['bbox_targets'].dtype == torch.float64
    assert torch.equal(dbl['grad_bbox'].float(), base['grad_bbox']) and torch.equal(dbl['label'].float(), base['label'])
    # scaled upstream gradients: one elementwise scale of the stored parts
    pos, gts, ious, rois, cls_score, bbox_pred = inputs
    tg = amd.pvrcnn_head_get_targets(pos, gts, ious, ref.CFG)
    x, p = cls_score.clone().requires_grad_(True), bbox_pred.clone().requires_grad_(True)
    losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, dict(ref.LOSS_BBOX, loss_weight=2.0), x, p, rois, *tg)
    (3.0 * losses['loss_cls'] + 0.5 * losses['loss_bbox'] + 0.0 * losses['loss_corner']).backward()
    assert torch.allclose(x.grad, 3.0 * base['grad_cls'], rtol=1e-6, atol=0)
    assert torch.allclose(p.grad, plain['grad_bbox'], rtol=1e-6, atol=1e-12)          # 0.5 x loss_weight 2
    assert torch.allclose(losses['loss_bbox'].detach(), 2.0 * base['loss_bbox'], rtol=1e-6)
    # a (R,) score and a bool mask are taken too
    l2 = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, cls_score.reshape(-1), bbox_pred, rois, tg[0], tg[1], tg[2], tg[3].bool(), tg[4], tg[5])
    assert all(torch.equal(l2[k], base[k]) for k in ref.LOSS_KEYS)


def test_double_backward_raises():
    pos, gts, ious, rois, cls_score, bbox_pred = ref.reference('r63', False)[0]
    tg = amd.pvrcnn_head_get_targets(pos, gts, ious, ref.CFG)
    p = bbox_pred.clone().requires_grad_(True)
    losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, cls_score, p, rois, *tg)
    (g,) = torch.autograd.grad(losses['loss_corner'] + losses['loss_bbox'], p, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()


class _Module:
    """a loss module stand-in: attributes instead of keys"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_argument_checks():
    pos, gts, ious, rois, cls_score, bbox_pred = ref.reference('r63', False)[0]
    tg = amd.pvrcnn_head_get_targets(pos, gts, ious, _Module(**ref.CFG))               # a config object
    args = (cls_score, bbox_pred, rois) + tuple(tg)
    ce = type('CrossEntropyLoss', (), {})()
    ce.__dict__.update(use_sigmoid=True, reduction='sum', loss_weight=1.0, class_weight=None)
    sl = type('SmoothL1Loss', (), {})()
    sl.__dict__.update(beta=1.0 / 9.0, reduction='sum', loss_weight=1.0)
    ok = amd.pvrcnn_head_loss(ce, sl, *args)                                           # modules, by class name and attributes
    assert torch.equal(ok['loss_bbox'], amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, *args)['loss_bbox'])
    with pytest.raises(RuntimeError, match='concat=True'):
        amd.pvrcnn_head_get_targets(pos, gts, ious, ref.CFG, concat=False)
    with pytest.raises(KeyError):
        amd.pvrcnn_head_get_targets(pos, gts, ious, dict(cls_pos_thr=0.75))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_head_get_targets(pos, gts + gts, ious, ref.CFG)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_head_get_targets([pos[0][:, :6]], [gts[0][:, :6]], ious, ref.CFG)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_head_get_targets([pos[0]], [gts[0][:-1]], ious, ref.CFG)
    with pytest.raises(RuntimeError, match='shape mismatch'):                           # more positives than RoIs in a sample
        amd.pvrcnn_head_get_targets([pos[0]], [gts[0]], [ious[0][:5]], ref.CFG)
    with pytest.raises(RuntimeError, match='must be a tensor'):
        amd.pvrcnn_head_get_targets([pos[0]], [gts[0]], [ious[0].tolist()], ref.CFG)
    with pytest.raises(RuntimeError, match='need pos_batch_cnt'):
        amd.pvrcnn_head_get_targets(pos[0], gts[0], ious[0], ref.CFG)
    with pytest.raises(RuntimeError, match='integer tensor'):
        amd.pvrcnn_head_get_targets(pos[0], gts[0], ious[0], ref.CFG, pos_batch_cnt=torch.tensor([20.0]), roi_batch_cnt=torch.tensor([63]))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_head_get_targets(pos[0], gts[0], ious[0], ref.CFG, pos_batch_cnt=torch.tensor([20, 0]), roi_batch_cnt=torch.tensor([63]))
    too_many = torch.zeros(1025, dtype=torch.int32)                                     # one sample more than MAX_SAMPLES: refused before any launch
    with pytest.raises(RuntimeError, match='too large'):
        amd.pvrcnn_head_get_targets(pos[0], gts[0], ious[0], ref.CFG, pos_batch_cnt=too_many, roi_batch_cnt=too_many)
    meta = torch.device('meta')
    with pytest.raises(RuntimeError, match='different devices'):
        amd.pvrcnn_head_get_targets([pos[0].to(meta)], gts, ious, ref.CFG)
    with pytest.raises(RuntimeError, match='is on'):
        amd.pvrcnn_head_get_targets(pos[0], gts[0], ious[0], ref.CFG, pos_batch_cnt=torch.tensor([20], device=meta), roi_batch_cnt=torch.tensor([63]))
    for bad in (dict(ref.LOSS_CLS, use_sigmoid=False), dict(ref.LOSS_CLS, reduction='mean'), dict(ref.LOSS_CLS, class_weight=[1.0]),
                dict(ref.LOSS_CLS, type='FocalLoss')):
        with pytest.raises(RuntimeError, match='loss_cls'):
            amd.pvrcnn_head_loss(bad, ref.LOSS_BBOX, *args)
    for bad in (dict(ref.LOSS_BBOX, reduction='mean'), dict(ref.LOSS_BBOX, type='L1Loss'), dict(ref.LOSS_BBOX, beta=0.0)):
        with pytest.raises(RuntimeError, match='loss_bbox|beta'):
            amd.pvrcnn_head_loss(ref.LOSS_CLS, bad, *args)
    for k, bad in ((0, cls_score[:-1]), (1, bbox_pred[:, :6]), (2, rois[:, 1:]), (3, tg[0][:-1]), (4, tg[1][:, :6]), (5, tg[2][:-1]),
                   (6, tg[3][:-1]), (7, tg[4][:-1]), (8, tg[5].reshape(-1, 1))):
        broken = list(args)
        broken[k] = bad
        with pytest.raises(RuntimeError, match='shape mismatch'):
            amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, *broken)
    with pytest.raises(RuntimeError, match='integer or bool'):
        amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, cls_score, bbox_pred, rois, tg[0], tg[1], tg[2], tg[3].float(), tg[4], tg[5])
    for k in (0, 2, 4, 6):
        broken = list(args)
        broken[k] = broken[k].to(meta)
        with pytest.raises(RuntimeError, match='is on'):
            amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, *broken)
    assert 'pvrcnn_head_get_targets' in amd.__all__ and 'pvrcnn_head_loss' in amd.__all__


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/roi_head_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/roi_head_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers on every edge shape, counts that overrun
    the rows, rows past the counts, null gradient pointers.  A sanitizer build belongs on a CPU-only machine: with a GPU present the
    test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    import os
    import subprocess
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'roi_head_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'roi_head_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'roi_head_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
