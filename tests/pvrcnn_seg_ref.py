"""tests/pvrcnn_seg_ref.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Torch restatement, statement by statement, of the two keypoint passages of the reference's PV-RCNN RoI head:
  PointwiseMaskHead.loss                 models/roi_heads/mask_heads/pointwise_mask_head.py:124-144
  the reweighting in _bbox_forward       models/roi_heads/pvrcnn_roi_head.py:211-212
with mmdet 2.x's FocalLoss(use_sigmoid=True) -> sigmoid_focal_loss -> py_sigmoid_focal_loss -> weight_reduce_loss restated from the
published text (mmdet is absent, its version not pinned — PARITY UNPINNED).  Runs in whatever dtype its inputs have (fp32: the
operation sequence a user runs at the parent commit; fp64: the yardstick); autograd gives the gradients.  Also the named cases of
tests/test_cpu_pvrcnn_seg.py and tests/test_gpu_pvrcnn_seg.py — every builder asserts its own preconditions — and one cached
evaluation per case that both files share (never modify the tensors)."""
import functools

import torch
import torch.nn.functional as F

NUM_CLASSES = 3
LOSS_SEG = dict(type='FocalLoss', use_sigmoid=True, reduction='sum', gamma=2.0, alpha=0.25, loss_weight=1.0)   # the shipped config
LOSS_RTOL = 1e-5           # the project's bar for a loss value (README)
NOISE_FACTOR = 4.0         # allowed multiple of the fp32 restatement's own deviation from fp64 (DESIGN.md §3.10's rule)
ULP = 2.0 ** -23           # one fp32 ulp of the tensor's largest magnitude: keeps an exactly rounded restatement from setting a bound of 0
LOGIT_LIMIT = 6.0          # parity cases: |x| <= 6 ...
TOP_GAP = 1e-3             # ... and every row's top two logits at least this far apart, so fp32 and fp64 pick the same column
INT64_EXTREMES = (2 ** 40, -2 ** 63, 2 ** 63 - 1)      # seg targets no 32-bit test can hold: weightless, like every target past background
INT64_EXTREME_ROWS = (11, 12, 13)                       # their rows in the `past_background` cases


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def py_sigmoid_focal_loss(pred, target, weight, gamma, alpha):
    """mmdet/models/losses/focal_loss.py, reduction='sum', avg_factor=None"""
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction='none') * focal_weight
    if weight.shape != loss.shape:
        weight = weight.view(-1, 1)             # weight.size(0) == loss.size(0): a weight per row
    loss = loss * weight                        # weight_reduce_loss
    return loss.sum()


def focal_loss(pred, target, weight, cfg):
    """FocalLoss.forward, use_sigmoid=True, not activated: the labels one-hot over pred's columns plus one, the last one dropped"""
    num_classes = pred.size(1)
    target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes]
    return cfg['loss_weight'] * py_sigmoid_focal_loss(pred, target, weight, cfg['gamma'], cfg['alpha'])


def seg_loss(seg_preds, seg_targets, num_classes, class_agnostic, cfg):
    """:124-144 -> (loss_seg, pos_normalizer).  One statement is added: a target above num_classes (F.one_hot would raise) is given the
    background label before one_hot; its weight pos + neg is 0 already."""
    pos_mask = (seg_targets > -1) & (seg_targets < num_classes)
    pos = pos_mask.to(seg_preds.dtype)
    neg = (seg_targets == num_classes).to(seg_preds.dtype)
    seg_weights = pos + neg
    pos_normalizer = pos.sum()
    seg_weights = seg_weights / torch.clamp(pos_normalizer, min=1.0)
    if class_agnostic:
        seg_cls_target = pos_mask.long()
    else:
        seg_cls_target = seg_targets.masked_fill(seg_targets < 0, num_classes)
        seg_cls_target = seg_cls_target.masked_fill(seg_cls_target > num_classes, num_classes)
    return focal_loss(seg_preds, seg_cls_target, seg_weights, cfg), pos_normalizer


def reweight(keypoints_feats, seg_preds):
    """:211-212 -> (reweighted features, the column max(dim) took)"""
    top = seg_preds.sigmoid().max(dim=-1, keepdim=True)
    return keypoints_feats * top.values, top.indices.reshape(-1)


# ---- the loss cases --------------------------------------------------------------------------------------------------------------

def _loss_case(n, agnostic, seed, kind='mixed', cfg=None):
    g = torch.Generator().manual_seed(seed)
    k = 1 if agnostic else NUM_CLASSES
    x = (torch.randn(n, k, generator=g) * 2).clamp(-LOGIT_LIMIT, LOGIT_LIMIT)
    if kind == 'mixed':            # ~25 % positives over the three classes, ~15 % ignored, the rest background; every kind present from 64 rows on
        u = torch.rand(n, generator=g)
        t = torch.full((n,), NUM_CLASSES, dtype=torch.int64)
        t[u < 0.25] = torch.randint(0, NUM_CLASSES, (n,), generator=g)[u < 0.25]
        t[u > 0.85] = -1
        if n >= 63:
            assert (t == -1).any() and (t == NUM_CLASSES).any() and all((t == c).any() for c in range(NUM_CLASSES))
    elif kind == 'one_positive':
        t = torch.tensor([1], dtype=torch.int64)
    elif kind == 'one_ignored':
        t = torch.tensor([-1], dtype=torch.int64)
    elif kind == 'no_positive':
        t = torch.where(torch.rand(n, generator=g) < 0.3, -1, NUM_CLASSES).to(torch.int64)
        assert (t == -1).any() and (t == NUM_CLASSES).any() and not ((t >= 0) & (t < NUM_CLASSES)).any()
    elif kind == 'all_ignored':
        t = torch.full((n,), -1, dtype=torch.int64)
    elif kind == 'past_background':
        t = torch.randint(-1, NUM_CLASSES + 1, (n,), generator=g)
        t[::5] = 4
        t[2::7] = 7
        for row, v in zip(INT64_EXTREME_ROWS, INT64_EXTREMES):     # rows that neither of the two strides above touches: no draw moves
            assert row % 5 != 0 and row % 7 != 2
            t[row] = v
        assert (t == 4).any() and (t == 7).any() and ((t >= 0) & (t < NUM_CLASSES)).any() and (t == NUM_CLASSES).any()
        assert all((t == v).any() for v in INT64_EXTREMES)
    elif kind == 'saturated':
        t = torch.randint(-1, NUM_CLASSES + 1, (n,), generator=g)
        x = torch.tensor([30.0, -30.0, 100.0, -100.0])[torch.randint(0, 4, (n, k), generator=g)]
        for v in (30.0, -30.0, 100.0, -100.0):      # each value on a positive and on a background row
            assert ((x == v).any(dim=1) & (t >= 0) & (t < NUM_CLASSES)).any() and ((x == v).any(dim=1) & (t == NUM_CLASSES)).any()
    else:
        raise KeyError(kind)
    assert t.shape == (n,) and x.shape == (n, k)
    if kind != 'saturated':
        assert float(x.abs().max()) <= LOGIT_LIMIT
    return dict(seg_preds=x, seg_targets=t, class_agnostic=agnostic, cfg=dict(cfg or LOSS_SEG))


def _loss_cases():
    cases = {}
    shapes = (('n1_pos', 1, 'one_positive'), ('n1_ignored', 1, 'one_ignored'), ('n63', 63, 'mixed'), ('n64', 64, 'mixed'), ('n65', 65, 'mixed'),
              ('n1023', 1023, 'mixed'), ('n1025', 1025, 'mixed'), ('n2049', 2049, 'mixed'),     # the wave edge; one, two, three chunks
              ('no_positive', 70, 'no_positive'), ('all_ignored', 65, 'all_ignored'), ('targets_past_background', 130, 'past_background'),
              ('saturated', 200, 'saturated'))
    for name, n, kind in shapes:
        for agnostic in (True, False):
            cases[f'{name}_{"k1" if agnostic else "k3"}'] = (n, agnostic, kind, None)
    for agnostic in (True, False):     # the general powf path
        cases[f'gamma_1p5_alpha_0p4_{"k1" if agnostic else "k3"}'] = (130, agnostic, 'mixed', dict(LOSS_SEG, gamma=1.5, alpha=0.4, loss_weight=0.7))
    return cases


LOSS_CASES = _loss_cases()


def make_loss(name):
    n, agnostic, kind, cfg = LOSS_CASES[name]
    return _loss_case(n, agnostic, 1000 + sorted(LOSS_CASES).index(name), kind, cfg)


def evaluate_loss(case, dtype):
    x = case['seg_preds'].to(dtype).clone().requires_grad_(True)
    loss, n_pos = seg_loss(x, case['seg_targets'], NUM_CLASSES, case['class_agnostic'], case['cfg'])
    loss.backward()
    return dict(loss=loss.detach(), n_pos=n_pos.detach(), grad=x.grad)


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    """(case, fp32 restatement, fp64 restatement), computed once and shared"""
    case = make_loss(name)
    return case, evaluate_loss(case, torch.float32), evaluate_loss(case, torch.float64)


# ---- the reweight cases ----------------------------------------------------------------------------------------------------------

def gapped_logits(n, k, g):
    """(n, k) logits in [-6, 6] whose top two of every row are at least 0.1 apart: uniform draws in [-6, 5.9], the row's largest moved up
    by 0.1 — no row has to be left out"""
    x = torch.rand(n, k, generator=g) * (2 * LOGIT_LIMIT - 0.1) - LOGIT_LIMIT
    x.scatter_add_(1, x.argmax(dim=1, keepdim=True), torch.full((n, 1), 0.1))
    return x


def check_gap(x):
    assert float(x.abs().max()) <= LOGIT_LIMIT
    if x.size(1) > 1:
        top = x.double().topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= TOP_GAP     # every row
        s = x.sigmoid().topk(2, dim=1).values
        assert float((s[:, 0] - s[:, 1]).min()) >= 2e-6             # the fp32 sigmoid separates them well above one ulp


def _reweight_case(n, c, k, seed, kind='parity'):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n, c, generator=g)
    grad_out = torch.randn(n, c, generator=g)
    x = gapped_logits(n, k, g)
    if kind == 'parity':
        check_gap(x)
    elif kind == 'exact_ties':
        assert k == 3 and n >= 12
        v = x.max(dim=1).values
        low = (v - 1.0).clamp(min=-LOGIT_LIMIT)
        x[0::4, 0], x[0::4, 1], x[0::4, 2] = v[0::4], v[0::4], low[0::4]    # columns 0 and 1 tie at the top
        x[1::4, 0], x[1::4, 1], x[1::4, 2] = low[1::4], v[1::4], v[1::4]    # columns 1 and 2
        x[2::4] = x[2::4].max(dim=1, keepdim=True).values.expand(-1, 3)     # all three
        check_gap(x[3::4])                                                  # every fourth row is an ordinary one
        assert (x[0::4, 0] == x[0::4, 1]).all() and (x[0::4, 2] < x[0::4, 0]).all() and (x[1::4, 0] < x[1::4, 1]).all()
        assert (x[2::4, 0] == x[2::4, 1]).all() and (x[2::4, 1] == x[2::4, 2]).all()
    elif kind == 'saturated':
        assert k == 1
        x = torch.tensor([30.0, -30.0, 100.0, -100.0])[torch.arange(n) % 4].reshape(n, 1)
    elif kind == 'forced_winner':
        # the row's largest logit — gapped_logits keeps it 0.1 above the next — changes places with the value of the column the row is
        # to pick: columns 0, K / 2 - 1, K / 2 (the first winner byte >= 128 at K = 255) and K - 1 in turn
        assert k >= 4
        want = torch.tensor(forced_columns(k))[torch.arange(n) % 4]
        top = x.argmax(dim=1)
        rows = torch.arange(n)
        hi, lo = x[rows, top].clone(), x[rows, want].clone()
        x[rows, top], x[rows, want] = lo, hi
        check_gap(x)
        assert torch.equal(x.argmax(dim=1), want) and torch.equal(x.double().argmax(dim=1), want)
    else:
        raise KeyError(kind)
    return dict(feats=feats, seg_preds=x, grad_out=grad_out)


def forced_columns(k):
    return (0, (k + 1) // 2 - 1, (k + 1) // 2, k - 1)


REWEIGHT_CASES = {
    'n1_c1_k1': (1, 1, 1, 'parity'),
    'n65_c3_k3': (65, 3, 3, 'parity'),            # the scalar path, C no multiple of 4
    'n65_c4_k1': (65, 4, 1, 'parity'),
    'n1025_c128_k1': (1025, 128, 1, 'parity'),    # the config's row form
    'n130_c128_k3': (130, 128, 3, 'parity'),
    'n67_c260_k3': (67, 260, 3, 'parity'),        # C past one wave of float4
    'n70_c132_k2': (70, 132, 2, 'parity'),        # C a multiple of 4, not of the lane group
    'exact_ties': (66, 8, 3, 'exact_ties'),
    'saturated': (64, 8, 1, 'saturated'),
}
# Cases added after the table above, with seeds of their own (the committed ones are indexed by sorted(REWEIGHT_CASES): they do not
# move): name -> (N, C, K, kind, seed).
#   The two sweeps are the smallest N at which a workgroup of reweight_kernel / reweight_backward_kernel takes a second trip of its
#   grid-stride loop: C = 256 and C = 255 are 64 quads, so group_lanes = 64 and a workgroup of 256 threads holds 256 / 64 = 4 rows;
#   the grid is capped at 8192 workgroups, so one sweep covers 8192 * 4 = 32768 rows and N = 32773 = 32768 + 5 leaves 5 rows to the
#   second trip — workgroup 0 takes four, workgroup 1 one (three of its four row slots are past N: in the backward those lanes still
#   reach the group shuffles), and every other workgroup's second trip does not start.  C = 256 takes the 16-byte path; C = 255 the
#   4-byte path, with the last quad of every row clipped to three columns.
#   K = 255 is the documented maximum: the winner is a byte, and columns 128 and 254 have its top bit set.
EXTRA_REWEIGHT_CASES = {
    'n32773_c256_k3': (32773, 256, 3, 'parity', 2501),
    'n32773_c255_k1': (32773, 255, 1, 'parity', 2502),
    'n130_c8_k255': (130, 8, 255, 'forced_winner', 2503),
}
SWEEP_CASES = ('n32773_c256_k3', 'n32773_c255_k1')
SWEEP_CAP, SWEEP_ROWS = 8192, 4                   # reweight_grid's cap and RW_BLOCK / group_lanes(C) of both sweep cases
for _name in SWEEP_CASES:
    assert EXTRA_REWEIGHT_CASES[_name][0] > SWEEP_CAP * SWEEP_ROWS and (EXTRA_REWEIGHT_CASES[_name][1] + 3) // 4 >= 64
ALL_REWEIGHT_CASES = sorted(REWEIGHT_CASES) + list(EXTRA_REWEIGHT_CASES)
MISALIGNED_OF = 'n130_c128_k3'                    # `misaligned_base`: this case's operands viewed one float into a larger buffer


def make_reweight(name):
    if name in EXTRA_REWEIGHT_CASES:
        n, c, k, kind, seed = EXTRA_REWEIGHT_CASES[name]
        return _reweight_case(n, c, k, seed, kind)
    n, c, k, kind = REWEIGHT_CASES[name]
    return _reweight_case(n, c, k, 2000 + sorted(REWEIGHT_CASES).index(name), kind)


def evaluate_reweight(case, dtype):
    f = case['feats'].to(dtype).clone().requires_grad_(True)
    x = case['seg_preds'].to(dtype).clone().requires_grad_(True)
    out, win = reweight(f, x)
    out.backward(case['grad_out'].to(dtype))
    return dict(out=out.detach(), win=win, grad_feats=f.grad, grad_seg=x.grad)


@functools.lru_cache(maxsize=None)
def reweight_reference(name):
    case = make_reweight(name)
    r32, r64 = evaluate_reweight(case, torch.float32), evaluate_reweight(case, torch.float64)
    assert torch.equal(r32['win'], r64['win']), 'the fp32 and fp64 restatements must pick the same column'
    return case, r32, r64


def offset_view(t):
    """t's values in a view that starts one float into a larger buffer: its base pointer is 4-byte aligned only"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- the bound -------------------------------------------------------------------------------------------------------------------

def bound(r32, r64):
    """(the fp32 restatement's largest deviation from fp64, the bound = the larger of NOISE_FACTOR times it and one fp32 ulp of the tensor's
    largest fp64 magnitude)"""
    if r64.numel() == 0:
        return 0.0, 0.0
    dev = float((r32.double() - r64).abs().max())
    return dev, max(NOISE_FACTOR * dev, ULP * float(r64.abs().max()))


def check_values(got, r32, r64, keys, what):
    """prints every measured figure, then asserts; returns {key: (error, fp32 restatement's deviation, bound)}"""
    figures, failures = {}, []
    for k in keys:
        assert got[k].shape == r64[k].shape and got[k].dtype == torch.float32, (k, got[k].shape, got[k].dtype)
        assert bool(torch.isfinite(got[k]).all()), f'{what}: {k} is not finite'
        dev, bnd = bound(r32[k], r64[k])
        err = float((got[k].double() - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f'{what} {k}: |ours - fp64| = {err:.3e}; fp32 restatement {dev:.3e}; bound {bnd:.3e}; ratio to bound {err / bnd if bnd else 0.0:.3f}')
        figures[k] = (err, dev, bnd)
        if not err <= bnd:
            failures.append((k, err, bnd))
    assert not failures, f'{what}: (key, error, bound) {failures}'
    return figures


def check_loss_value(got, r64, what):
    want = float(r64)
    err = abs(float(got) - want)
    print(f'{what} loss: ours {float(got):.9g}, fp64 {want:.9g}, relative error {err / abs(want) if want else err:.3e} (bar {LOSS_RTOL:g})')
    assert err <= LOSS_RTOL * abs(want), (what, float(got), want)
